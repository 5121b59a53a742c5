// csrc/flat_collect.h -- shared by the coarse-filter scan kernels (flat_collect.hip: d <= 128; flat_collect_wide.hip: 128 < d <= 1536)
#pragma once

// ---- the schedule of the d <= 128 scan (DESIGN.md 3.1 "persistent scan"): plain C++, no HIP -- tests/test_scan_ranges_cpu.py compiles
// this part alone (MVS_COLLECT_PLAN_ONLY) into a program of its own --------------------------------------------------------------------
// The scan is a persistent kernel: at most one workgroup per resident slot, each pulling items (row range, query block) until the
// queues are empty.  The rows are cut into RANGES of whole stages: a body of equal ranges of roughly the size the one-shot launch used
// (at least CL_BODY_MIN_ROWS rows, at most CL_BODY_MAX_RANGES of them), then, for the last part of the store, ranges that halve from
// level to level down to a floor -- so the last items handed out are short and all slots run dry within a short time of each other.
// A size is used as long as more than CL_TAPER_ROUNDS rounds of the slots, at that size, are left for the smaller ones ("factoring").
// Equal sizes are consecutive, so the plan is a few LEVELS {first range, rows per range, first row}: it travels in the kernel's
// arguments, and nothing is uploaded or cached per search.
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define MVS_PLAN_HD __host__ __device__ // (the scan kernel's take() calls collect_queue_items: one definition, the one the CPU test checks)
#else
#define MVS_PLAN_HD
#endif

namespace mvs {

constexpr int CL_SCHED_LEVELS = 12;      // levels a plan can hold: the body + at most ten halvings + the floor
constexpr int CL_BODY_MIN_ROWS = 7680;   // the one-shot planner's floor for a row split
constexpr int CL_BODY_MAX_RANGES = 384;  // ... and the number of splits it chose at the headline (N = 10 M: 26 112 rows)
constexpr int CL_TAPER_ROUNDS = 2;       // taper's share: rounds of the slots kept for the sizes below (profiles/scan_schedule_ab.txt)
constexpr int CL_TAPER_FLOOR_ROWS = 512; // ... and its floor: four int8 stages, eight bf16 ones (same table)
constexpr unsigned CL_ITEM_NONE = 0xffffffffu; // "the queues are empty" where a workgroup expects an item

struct CollectSched {
	int nlev, nranges;
	int first[CL_SCHED_LEVELS];       // the level's first range
	int rows[CL_SCHED_LEVELS];        // rows per range of the level (a multiple of the stage; the store's last range ends at its last row)
	long long begin[CL_SCHED_LEVELS]; // the level's first row, from the scan's first row
};

// Ranges over n_rows rows for nqb query blocks on `slots` resident workgroups.  Contiguous from 0 to n_rows, every boundary but the end a
// multiple of stage_rows, sizes never increasing, at most CL_BODY_MAX_RANGES + 2 CL_SCHED_LEVELS CL_TAPER_ROUNDS (slots / nqb + 1) ranges.
inline CollectSched collect_plan_levels(int64_t n_rows, int64_t stage_rows, int64_t nqb, int64_t slots) {
	CollectSched s = {};
	if (n_rows <= 0 || stage_rows <= 0)
		return s;
	if (nqb < 1)
		nqb = 1;
	const int64_t total = (n_rows + stage_rows - 1) / stage_rows; // stages
	int64_t nbody = n_rows / CL_BODY_MIN_ROWS;
	nbody = nbody < 1 ? 1 : (nbody > CL_BODY_MAX_RANGES ? CL_BODY_MAX_RANGES : nbody);
	const int64_t body = (total + nbody - 1) / nbody;             // stages per range of the body
	const int64_t per_round = (slots + nqb - 1) / nqb;            // ranges whose items fill every slot once
	int64_t floor_st = (CL_TAPER_FLOOR_ROWS + stage_rows - 1) / stage_rows;
	if (floor_st < (body + 511) / 512) // (a huge store: ten halvings reach the floor)
		floor_st = (body + 511) / 512;
	int64_t rem = total, size = body, done = 0, nr = 0;
	while (rem > 0) {
		const bool last = size <= floor_st || s.nlev == CL_SCHED_LEVELS - 1;
		int64_t count;
		if (last) {
			count = (rem + size - 1) / size;
		} else {
			const int64_t keep = (int64_t)CL_TAPER_ROUNDS * per_round * size; // stages left to the smaller sizes
			count = rem > keep ? (rem - keep + size - 1) / size : 0;
			if (count > rem / size)
				count = rem / size;
		}
		if (count > 0) {
			s.first[s.nlev] = (int)nr;
			s.rows[s.nlev] = (int)(size * stage_rows);
			s.begin[s.nlev] = done * stage_rows;
			++s.nlev;
			nr += count;
			done += count * size;
			rem = last ? 0 : rem - count * size;
		}
		size = (size + 1) / 2 > floor_st ? (size + 1) / 2 : floor_st;
	}
	s.nranges = (int)nr;
	return s;
}
// the same as boundaries: range r = [b[r], b[r + 1]), b.back() = n_rows
inline std::vector<int64_t> collect_plan_ranges(int64_t n_rows, int64_t stage_rows, int64_t nqb, int64_t slots) {
	const CollectSched s = collect_plan_levels(n_rows, stage_rows, nqb, slots);
	std::vector<int64_t> b;
	for (int l = 0; l < s.nlev; ++l) {
		const int end = l + 1 < s.nlev ? s.first[l + 1] : s.nranges;
		for (int r = s.first[l]; r < end; ++r)
			b.push_back(s.begin[l] + (int64_t)(r - s.first[l]) * s.rows[l]);
	}
	b.push_back(n_rows > 0 ? n_rows : 0);
	return b;
}
// Range r belongs to the queue of XCD r & 7; a queue's items are range-major, query-block-minor (workgroups that run at the same time
// stream the same rows through one L2): item j of queue x = range 8 (j / nqb) + x, query block j % nqb
MVS_PLAN_HD inline int64_t collect_queue_items(int nranges, int x, int64_t nqb) {
	return nranges > x ? (int64_t)((nranges - x + 7) >> 3) * nqb : 0;
}

// ---- upkeep of the running bound, paced by progress (DESIGN.md 3.1 "bound upkeep") -----------------------------------------------------
// A workgroup of the scan re-derives its query block's pass bounds from the class slots every `derive` stages and fetches the block's
// shared table every `fetch` stages.  The bound moves like the logarithm of the rows seen, so a fixed cadence is sized to the first
// percent of the scan and repeated for the other 99: instead, the periods of an item follow the rows the grid had behind it when the
// item was handed out.  Items go out range-major and slots / nqb ranges are at work at a time, so those rows are the first row of range
// rng - ceil(slots / nqb) (none for the first round).  A workgroup derives once per 1 / CL_UPKEEP_SHARE of them -- the table of a query
// block, refreshed in turn by the workgroups that share it (the phase below), is then never staler than that share of what was seen --
// between a floor and a ceiling; the period doubles when the rows seen double.  The table is fetched CL_UPKEEP_FETCH_DIV times per
// derivation period, no more often than the bf16-era 256 rows.
// (the constants by measurement, profiles/scan_classes_ab.txt: a derivation costs far more than the admissions a staler bound lets in)
constexpr int CL_UPKEEP_FLOOR_ROWS = 8192;   // derivation period at the start: 64 stages of the int8 store
constexpr int CL_UPKEEP_CEIL_ROWS = 131072;  // ... and at most: 1024 stages
constexpr int CL_UPKEEP_SHARE = 4;
constexpr int CL_UPKEEP_FETCH_DIV = 32;
constexpr int CL_UPKEEP_FETCH_FLOOR_ROWS = 256;
struct CollectUpkeep {
	int derive, fetch; // periods in stages, powers of two
};
MVS_PLAN_HD inline CollectUpkeep collect_upkeep_periods(long long seen_rows, int stage_rows) {
	CollectUpkeep up;
	const int ceil_st = CL_UPKEEP_CEIL_ROWS / stage_rows;
	up.derive = CL_UPKEEP_FLOOR_ROWS / stage_rows;
	while (up.derive < ceil_st && 2ll * up.derive * stage_rows * CL_UPKEEP_SHARE <= seen_rows)
		up.derive *= 2;
	up.fetch = CL_UPKEEP_FETCH_FLOOR_ROWS / stage_rows;
	while (up.fetch * 2 * CL_UPKEEP_FETCH_DIV <= up.derive)
		up.fetch *= 2;
	return up;
}
// the first row of range r of a plan, from the scan's first row (S: CollectSched wherever it lies -- the kernel reads it in its argument segment)
template <class S> MVS_PLAN_HD inline long long collect_range_begin(const S *p, int r) {
	const int nlev = p->nlev;
	int lev = 0;
	for (int l = 1; l < nlev && r >= p->first[l]; ++l) // the range's level: equal sizes are consecutive
		lev = l;
	return p->begin[lev] + (long long)(r - p->first[lev]) * p->rows[lev];
}
// rows behind the grid when range rng is handed out to one of `slots` workgroups
template <class S> MVS_PLAN_HD inline long long collect_seen_rows(const S *p, int rng, int nqb, int slots) {
	const int at_work = (slots + nqb - 1) / nqb;
	return rng > at_work ? collect_range_begin(p, rng - at_work) : 0;
}
// does stage u of an item of range rng derive?  The workgroups of a query block work on consecutive ranges: the phase makes them take turns
MVS_PLAN_HD inline bool collect_upkeep_due(int u, int rng, int derive) {
	return ((u + rng * 13 + 5) & (derive - 1)) == 0;
}

// ---- the layout of a query block (DESIGN.md 3.1 "a wave's share"): which tile columns a wave of the scan's workgroup works on ------------
// A query block is CL_QCOLS tile columns of 32 queries, a workgroup four waves, and a wave holds the fragments of four tile columns in its
// four SLOTS (slot = place in the wave's registers and in its part of the bound table, [wave][slot][16][2]).  A stage is `sub_tiles` row tiles
// of 32 rows (4 on the int8 store, 2 on bf16), so a block with T live columns has T * sub_tiles (column, row tile) jobs per stage.
//   T = 16 (a full block): wave w owns columns 4 w .. 4 w + 3 on every row tile -- sixteen jobs per wave and stage on the int8 store.
//   T < 16: every wave OWNS T / 4 columns (wave w: (T / 4) w + t in slot t) on every row tile, and the r = T % 4 columns behind them,
//   4 (T / 4) + j, are SHARED: several waves hold such a column in a slot behind their own ones and each runs it on some of the stage's row
//   tiles only, so that every job is done once and the work comes off all four waves evenly (the waves of a CU meet at the stage barriers:
//   idle waves would leave their SIMDs short while the busy ones still set the pace).
//     int8 store, r <= 4 - T / 4: all four waves hold all r shared columns and wave w runs them on row tile w: T jobs per wave and stage.
//     int8 store, T = 14 / T = 11 (more shared columns than free slots): the waves share in pairs -- column 4 (T / 4) + p belongs to waves
//     2 p and 2 p + 1, which run it on row tiles {0, 1} and {2, 3}; at T = 11 the third column is held by all four, each on one row tile of
//     its two.  T jobs per wave and stage as well.
//     T = 15 cannot be done in fewer than sixteen jobs by every wave with four slots each (fifteen columns in sixteen slots: all but one
//     column have a single holder, which runs all their row tiles; a wave that holds four such columns does sixteen jobs): the full layout.
//     bf16 store (two row tiles per stage): the full layout for every block.  Shared columns there (a column to two waves, one row tile
//     each) returned the same results but admitted a quarter more candidates at 128 row classes and overflowed the stream of
//     tests/test_collect_gpu.py's k = 128 case; the cause is not understood, so that store keeps what it had.
// A wave's shared slots run on nested sets of row tiles (what runs slot t + 1 runs slot t), so on row tile s it runs slots 0 .. n(s) - 1 and
// the kernel leaves the tile-column loop at n(s).  A free slot names column 15, which has no live query in a partial block.
// The word: bits 4 t .. 4 t + 3 = the column of slot t; bits 16 + 3 s .. 18 + 3 s = n(s), s < sub_tiles.
constexpr int CL_QCOLS = 16; // tile columns of a query block (CL_QBLOCK = 32 CL_QCOLS queries)
constexpr unsigned CL_QLAYOUT_FULL_N = 0x924u; // the word's n(s) part (bits 16 ..) of the full layout, and of no other: n(s) = 4 for every s
MVS_PLAN_HD inline int collect_qblock_cols(int nq, int qb) { // T: live tile columns of block qb
	const int live = nq - qb * 32 * CL_QCOLS;
	return live >= 32 * CL_QCOLS ? CL_QCOLS : (live <= 0 ? 0 : (live + 31) >> 5);
}
MVS_PLAN_HD inline unsigned collect_qblock_wave(int nq, int qb, int sub_tiles, int wave) {
	const int T = collect_qblock_cols(nq, qb);
	const int own = T >> 2, r = T & 3, spare = 4 - own;
	if (T == CL_QCOLS || sub_tiles != 4 || (r == 3 && spare == 1)) // full (and T = 15, and the bf16 store)
		return (unsigned)(4 * wave) * 0x1111u + 0x3210u + (CL_QLAYOUT_FULL_N << 16); // columns 4 w + t, n(s) = 4
	const int pair = wave >> 1, half = wave & 1;
	// (words, not arrays: the scan kernel decodes an item with this, in scalar registers)
	unsigned cols = 0xFFFFu;        // a nibble per slot
	unsigned n = 0x249u * (unsigned)own; // three bits per row tile
#define MVS_QB_PUT(slot, col) cols = (cols & ~(15u << (4 * (slot)))) | ((unsigned)(col) << (4 * (slot)))
	for (int t = 0; t < own; ++t)
		MVS_QB_PUT(t, own * wave + t);
	if (r <= spare) {
		for (int j = 0; j < r; ++j)
			MVS_QB_PUT(own + j, 4 * own + j);
		n += (unsigned)r << (3 * wave);
	} else { // T = 14, 11
		MVS_QB_PUT(own, 4 * own + pair);
		n += 9u << (6 * half); // row tiles 2 half and 2 half + 1
		if (r == 3) {
			MVS_QB_PUT(own + 1, 4 * own + 2);
			n += 1u << (3 * (2 * half + pair));
		}
	}
#undef MVS_QB_PUT
	return cols | n << 16;
}
MVS_PLAN_HD inline int collect_qblock_slot_col(unsigned word, int slot) { // the tile column of a slot: its first query is qb * 512 + 32 * this
	return (int)((word >> (4 * slot)) & 15u);
}
MVS_PLAN_HD inline int collect_qblock_ncols(unsigned word, int row_tile) { // n(s): the wave runs slots 0 .. n(s) - 1 on row tile s of a stage
	return (int)((word >> (16 + 3 * row_tile)) & 7u);
}

// device words of the schedule (behind the bound table: collect_bound_table_bytes): eight cursors and the count of finished workgroups,
// each on a 128-byte line of its own
constexpr int CL_CURSOR_STRIDE = 32; // unsigned words
constexpr size_t CL_CURSOR_BYTES = 9 * CL_CURSOR_STRIDE * 4;

} // namespace mvs

#ifndef MVS_COLLECT_PLAN_ONLY
#include "flat_fused.h"

#include <cstddef>

namespace mvs {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4n __attribute__((ext_vector_type(4)));
typedef float f32x2n __attribute__((ext_vector_type(2)));
typedef int i32x4n __attribute__((ext_vector_type(4))); // 16 int8 of an int8 MFMA fragment, or 4 i32 of its accumulator
typedef int i32x2n __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) float lds_f32c;
typedef __attribute__((address_space(1))) const float glb_f32c;

constexpr int CL_QBLOCK = 512;  // queries per workgroup
constexpr int CL_BN = 32;       // rows per tile (one pass of the MFMA loop)
constexpr double CL_MFMA_UNITS = 8.0; // modelled bf16-MFMA accumulation error, ulp-units (2^-24) of the magnitudes per 16 dimensions (csrc/flat_collect.hip)
constexpr int CL_SUB = 2;       // tiles per staged block (one barrier per CL_SUB tiles)
constexpr int CL_SUB_I8 = 4;    // ... of the d <= 128 scan on the int8 store (csrc/flat_collect.hip: a stage of 128 rows, 16 KB as on bf16)
constexpr int cl_sub(bool i8) { return i8 ? CL_SUB_I8 : CL_SUB; }
constexpr int CL_QCAP = 2048;   // candidate queue of a workgroup (entries of 8 bytes)
// ... of the d <= 128 scan: half of it on the int8 store, whose 16 KB stages of 128 rows and three workgroups per CU leave 54 613 B each
constexpr int cl_qcap(bool i8) { return i8 ? CL_QCAP / 2 : CL_QCAP; }
constexpr int CL_FLUSH_EVERY = 2; // staged blocks between two looks at the queue
constexpr int CL_FROZEN = 256;  // CollectArgs::flags (bit 8, where it sat among the retired A/B bits: the kernels that test it compile as before)

struct CollectArgs {
	const void *qf;            // query fragments (bf16), [qblk32][ch][lane] x 16 bytes
	const unsigned short *yb;  // bf16 rows [n + 64][dp]
	const float *yn;           // beta(row): -||y'||^2 (L2) or <mu, y> (inner product), f32, padded by 64
	const float *e2;           // [nq] 2E(q) (NaN: the query is not served here)
	unsigned *gslot;           // [nq][slot_stride] class slots: keys of the best s per row class (smaller key = better)
	unsigned long long *stream; // candidates (q << 32 | row)
	unsigned long long *stream_cnt; // [0] entries appended
	float *stream_s;           // (may be null; d <= 128 scan) the coarse value s of every entry: the final-bound filter's input
	float *seed_stage;         // (flat_bf16_seed_kernel) [nsplit][nq][16] class maxima of every row split
	const unsigned long long *rowmask; // SEL instances: bit r of word b = row 64 b + r passes the IDSelector
	long long stream_cap;
	int slot_stride, nclass; // 16 class slots per query (row & 15); nclass = kk, the rank of the bound among them
	long long n, row_first, split_rows;
	long long split_len; // flat_bf16_seed_kernel: rows of a split actually scanned (0: split_rows) -- pass A of the big lists strides over the database
	int nq, nqb, nsplit, xcd_map;
	float *pbnd; // d <= 128 scan: [nqb][512] pass bounds B - 2E in the order of a workgroup's LDS table (flat_collect.hip), or null
	int flags; // CL_FROZEN: the bounds in pbnd come from a pass of their own and are never re-derived (big lists: launch_collect_big_bounds)
	float i8_unit; // > 0: yb / yn are the int8 store (int8 rows, i32 beta_int) and s = s_int * i8_unit (a power of two); 0: the bf16 store
	unsigned *cursors; // d <= 128 scan: the item queues' cursors and the count of finished workgroups (collect_cursors; zero between launches)
};
// The one argument of flat_bf16_collect_kernel: the kernel reads the plan where it lies in the argument segment, offsetof(CollectLaunch, sc)
struct CollectLaunch {
	CollectArgs a;
	CollectSched sc;
};

// int8 store: the integer pass bound of a real one -- the smallest n with n * unit >= p (p * inv_unit and its ceiling are exact for
// unit = 2^k), so the integer test s_int >= n admits exactly the rows the real test s >= p admits.  NaN -> INT_MAX (nothing passes:
// |s_int| < 2^24); clamped to [-(2^31 - 1), 2^31 - 1] so that the outlier rows' beta_int = INT_MIN never passes.
__device__ __forceinline__ int cl_i8_thr(float p, float inv_unit) {
	const float t = ceilf(p * inv_unit);
	if (!(t == t) || t > 1073741824.f)
		return 0x7fffffff;
	if (t < -1073741824.f)
		return -0x7fffffff;
	return (int)t;
}

// csrc/flat_collect_wide.hip
int collect_store_dims(int d); // row pitch (dims) of the bf16 store: 128, 256, 384, 512, 768, 1024; 0 = the coarse filter does not serve d
int collect_wide_qblock(int dp1);
int collect_wide_slots(int dp1);
int collect_wide_max_classes(int dp1); // row classes per query the wide store's kernel can keep: 128 (wide / big kernels: 16 | 32 | 4 x 32)
size_t collect_wide_lds_bytes(int dp1);
int collect_wide_block_rows(int dp1);
void launch_collect_wide_range(int dp1, int metric, bool collect, CollectArgs a, int64_t row_first, int64_t row_end,
                               int64_t nsplit_want, int64_t nq, hipStream_t st, int *grid_out, int *nsplit_out);
// csrc/flat_collect_big.hip: 512 < d <= 1024, one wave per SIMD with all of k resident (512 registers per wave)
int collect_big_qblock(int dp1);
size_t collect_big_lds_bytes(int dp1);
void launch_collect_big(int dp1, int metric, bool collect, const CollectArgs &a, int grid, hipStream_t st);
void launch_rows_to_bf16_wide(int metric, const float *d_vecs, int sdp, int interleaved, int d, int dp1, int64_t row0, int64_t nrows,
                              const float *d_mu, unsigned short *d_bf, float *d_beta, const float *d_norms,
                              unsigned *d_max_norm_bits, hipStream_t st, int *d_outl);
void launch_collect_exact_wide(int metric, bool per_pair, unsigned long long *d_sorted, int64_t ncand, const float *d_x, int d,
                               const float *d_vecs, int sdp, int interleaved, const float *d_norms, const float *d_qn, hipStream_t st,
                               const unsigned long long *d_cnt = nullptr);

// ---- what the HOST reads and addresses of the coarse filter's device state (csrc/flat_coarse.hip, csrc/index.hip) -----------------------
// The kernels address these fields by the same numbers, written out; a field that moves moves there too.
// Control block of a search (FlatIndex::ws_seg): this header, then [nq] ints -- the segment table of the sorted pipeline or the bucket
// counters of the bucketed finish.  collect_query_prep_kernel (the wide stores: a memset) zeroes header and table.
struct CollectCtl {
	unsigned long long count; // entries the scan appended to the candidate stream, beyond its capacity too (scan kernels, collect_append_outliers_kernel)
	unsigned long long kept;  // survivors of the final-bound filter (csrc/ivf_collect.hip ivf_bucket_select_kernel: kept_out; launch_stream_refilter: d_out_cnt)
	unsigned units;           // work units of the bucket scatter (csrc/ivf_collect.hip ivf_bucket_scatter_kernel: unit_cnt)
	unsigned pad0_[43];
	unsigned long long bucket_stats; // the bucket finish's statistics (csrc/ivf_collect.hip ivf_bucket_select_kernel: stats[0]) ...
	unsigned long long bucket_max;   // ... stats[1]: the most survivors any query had for its bucket (> the pitch: that bucket overflowed)
	unsigned long long pad1_[6];
};
static_assert(sizeof(CollectCtl) == 256 && offsetof(CollectCtl, kept) == 8 && offsetof(CollectCtl, units) == 16 &&
                  offsetof(CollectCtl, bucket_stats) == 192 && offsetof(CollectCtl, bucket_max) == 200,
              "the kernels address the control block by these offsets");
inline int *collect_ctl_table(void *ctl) { // the per-query table behind the header
	return (int *)((CollectCtl *)ctl + 1);
}
// Pinned report of a search (FlatIndex::h_report, 64 bytes): collect_report_kernel writes [8] .. [11] as ints
struct CollectReport {
	int tie_flags;                 // [0] FlatIndex::resolve_ip_ties' copy of TieFlags::count
	int pad0_[7];
	int fail_count;                // [8] queries without a proven candidate set (re-run on the exact kernels)
	float residual;                // [9] the word of d_max_norm_bits at CL_NORM_REL_ERR
	unsigned long long candidates; // [10..11] CollectCtl::count (deferred count mode: the report kernel; else a copy behind the scan)
	int pad1_[4];
};
static_assert(sizeof(CollectReport) == 64 && offsetof(CollectReport, fail_count) == 32 && offsetof(CollectReport, residual) == 36 &&
                  offsetof(CollectReport, candidates) == 40,
              "collect_report_kernel writes the report by these offsets");
// Words of FlatIndex::d_max_norm_bits (f32 bits, atomicMax; rows_to_bf16 kernels of csrc/flat_collect.hip, csrc/flat_collect_wide.hip, csrc/flat_bf16.hip)
constexpr int CL_NORM_ROWS = 0;      // largest ||y||^2 of the original rows
constexpr int CL_NORM_STORE = 2;     // ... of the rows that are in the coarse store (not the outliers)
constexpr int CL_NORM_TAU = 3;       // the outlier threshold tau (collect_outlier_threshold_kernel; +inf: no outlier handling)
constexpr int CL_NORM_REL_ERR = 4;   // largest |approx - exact| / (||x|| ||y||) of a re-scored candidate (csrc/flat_bf16.hip rescore_verify_kernel)
constexpr int CL_NORM_CENTRED = 8;   // largest ||y - mu||^2
constexpr int CL_NORM_RESIDUAL = 12; // largest ||y' - bf16(y')||^2 of the centred rows
// Words of FlatIndex::d_i8_bits (f32 bits; rows_to_i8_kernel of csrc/flat_collect.hip)
constexpr int CL_I8_RESIDUAL = 0; // max ||y' - sy Y||^2
constexpr int CL_I8_BETA_MAX = 1; // max |beta / unit|
constexpr int CL_I8_ABS_MAX = 2;  // max |y'_i|

__device__ __forceinline__ unsigned skey(float s) { // "larger s is better" as a smaller-is-better key
	return ~f2key(s);
}
__device__ __forceinline__ float skey2f(unsigned k) {
	return key2f(~k);
}

} // namespace mvs

#endif // MVS_COLLECT_PLAN_ONLY
