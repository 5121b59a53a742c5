// csrc/collect_launch.h -- host interface of the coarse-filter family: what csrc/flat_coarse.hip, csrc/index.hip and csrc/ivf.hip call in
// csrc/flat_collect.hip, csrc/flat_collect_wide.hip, csrc/ivf_collect.hip, csrc/coarse_bf16.hip and csrc/coarse_select.hip.
// The argument structs are plain host data with default member initialisers: a call site names the fields it uses and leaves the
// others alone.  The launchers copy them into the kernels' own argument structs (CollectArgs, IvfBucketSelectArgs, ...).
#pragma once
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace mvs {

// ---- shared operands ------------------------------------------------------------------------------------------------------------------
// The candidate stream a scan appends to and the finishes read
struct CandStream {
	unsigned long long *entries = nullptr; // q << 32 | row
	float *values = nullptr;               // (may be null) the coarse value of every entry: the final-bound filters' input
	unsigned long long *count = nullptr;   // [0] entries appended, beyond the capacity too
	int64_t cap = 0;
};
// Queries the coarse filter cannot serve go here and are re-run on the exact kernels
struct FailList {
	int *count = nullptr;
	int *queries = nullptr;
};

// ---- csrc/flat_collect.hip: the stores ------------------------------------------------------------------------------------------------
bool collect_supported(const FlatGeom &g);
void launch_collect_mean(const FlatGeom &g, const float *d_vecs, int64_t nrows, float *d_mu, hipStream_t st);
// rows [row0, row0 + nrows) of the f32 store -> the centred bf16 store (d <= 128) and beta
struct CollectStoreRows {
	int metric = 0;
	const float *vecs = nullptr;
	int64_t row0 = 0, nrows = 0;
	const float *mu = nullptr;
	unsigned short *bf = nullptr;
	float *beta = nullptr;
	const float *norms = nullptr;
	unsigned *max_norm_bits = nullptr;
	int *outl = nullptr; // (may be null) the outlier rows' list
};
void launch_rows_to_bf16_hi(const FlatGeom &g, const CollectStoreRows &r, hipStream_t st);
// the int8 coarse store (csrc/flat_collect.hip "int8 store"): range = true measures max |y'_i| into bits[2] only
struct CollectI8Rows {
	bool range = false;
	const float *vecs = nullptr;
	int64_t row0 = 0, nrows = 0;
	const float *mu = nullptr, *beta = nullptr;
	float sy = 0.f, unit = 0.f;
	signed char *i8 = nullptr;
	int *beta_i = nullptr;
	unsigned *bits = nullptr;
};
void launch_rows_to_i8(const FlatGeom &g, const CollectI8Rows &r, hipStream_t st);
// outlier rows of the coarse-filter store (csrc/flat_collect.hip "outlier rows")
void launch_collect_outlier_threshold(const float *d_norms, int64_t nrows, const float *d_mu, int dp, unsigned *d_max_norm_bits, hipStream_t st);
void launch_collect_append_outliers(const int *d_outl, int n_outliers, int64_t nq, const CandStream &s, const unsigned long long *d_rowmask,
                                    hipStream_t st);
size_t collect_qfrag_bytes(const FlatGeom &g, int64_t nq);
const char *collect_wide_kernel_name(int dp1); // "flat_bf16_big_kernel" / "flat_bf16_wide_kernel" for a store pitch > 128
size_t collect_qfrag_bytes_ex(int dp1, int qblock, int64_t nq);
// class slots per query: 16 | 32 | 128 (kk > 32; wide stores: where the kernel has the instance).  i8: the pass runs on the int8 store,
// which keeps 32 classes from kk = CL_I8_CLASSES32_FROM on (DESIGN.md 3.1 "row classes")
constexpr int CL_I8_CLASSES32_FROM = 15;
int collect_slot_stride(int kk, int dp1, bool i8);
int collect_max_k(int d); // largest k (+1 with tie detection) the coarse filter serves at this d: 128, or 0

// ---- csrc/flat_collect.hip: the queries of a search -----------------------------------------------------------------------------------
// launch_collect_query_prep (d <= 128 store): fragments, ||x||^2, 2E, neutral class slots and the zeroed control block in one launch.
// The wide stores fill the same struct for launch_collect_pack_queries_ex (x, mu -> qf) and launch_collect_bounds (-> e2, fail).
struct CollectQueryPrep {
	int metric = 0;
	const float *x = nullptr;
	int64_t nq = 0;
	int d = 0;
	const float *mu = nullptr;
	const unsigned *max_norm_bits = nullptr;
	void *qf = nullptr; // fragments: nq rounded up to the scan's query block
	float *qn = nullptr;
	float *e2 = nullptr; // (nq rounded up to 256) entries
	FailList fail;
	unsigned *gslot = nullptr; // (may be null, stride 0: no class slots)
	int stride = 0;
	int *ctl_hdr = nullptr, *ctl_seg = nullptr;
	const unsigned *i8_bits = nullptr;
	float i8_sa = 0.f, i8_unit = 0.f; // i8_unit > 0: fragments and E for the int8 store
	unsigned *cursors = nullptr;      // the persistent scan's cursors: zeroed with the control block
};
void launch_collect_query_prep(const CollectQueryPrep &p, hipStream_t st);
void launch_collect_pack_queries_ex(const CollectQueryPrep &p, int dp1, int qblock, hipStream_t st);
void launch_collect_bounds(const CollectQueryPrep &p, hipStream_t st);
size_t collect_bound_table_bytes(int64_t nq);
unsigned *collect_cursors(float *d_pbnd, int64_t nq); // the persistent scan's item cursors, behind the bound table
size_t collect_rowmask_bytes(int64_t n);
void launch_collect_rowmask(SelectorDev sel, const int64_t *d_idmap, int64_t n, unsigned long long *d_mask, hipStream_t st);

// ---- csrc/flat_collect.hip: one pass over the store -----------------------------------------------------------------------------------
// What the pre-pass, the big lists' pass A and the scan have in common
struct CollectPass {
	FlatGeom g;
	int metric = 0;
	const void *qf = nullptr;
	const unsigned short *rows = nullptr; // the bf16 store, or (i8_unit > 0) the int8 store's rows ...
	const float *beta = nullptr;          // ... and beta_int
	int64_t n = 0, nq = 0;
	int kf = 0;
	const float *e2 = nullptr;
	unsigned *gslot = nullptr;
	const unsigned long long *rowmask = nullptr;
	float *pbnd = nullptr; // the d <= 128 scan's bound table, or null
	float i8_unit = 0.f;
	int classes = 0; // option cl_classes (tests): 16 | 32 = the int8 store's row classes for kk <= 16 whatever the rule says; 0: the rule
	hipStream_t st = nullptr;
};
int collect_pass_stride(const CollectPass &p); // collect_slot_stride of the pass: every launcher and the index's plan use this one
// slots -> neutral, stream counter -> 0, then the bound-estimation pre-pass over the first rows
struct CollectPrepare {
	unsigned long long *stream_cnt = nullptr;
	bool cnt_zeroed = false, slots_ready = false;
	float *seed_stage = nullptr; // collect_seed_stage_bytes; the d <= 128 store only
};
void launch_collect_prepare(const CollectPass &p, const CollectPrepare &pr);
size_t collect_seed_stage_bytes(int64_t nq, int nc); // [64][nq][nc] floats: the register pre-pass's class maxima per row split (csrc/flat_collect.hip)
// the main scan: every row, candidates into the stream.  frozen: the bounds in p.pbnd come from pass A and are never re-derived
struct CollectScanInfo {
	int grid = 0, nsplit = 0, lds = 0; // (d <= 128: nsplit = row ranges of the plan ...
	int64_t items = 0;                 // ... items = ranges x query blocks)
};
CollectScanInfo launch_collect_scan(const CollectPass &p, const CandStream &s, bool frozen);
// lists beyond 128 entries: pass A -- T - 2E per query from `ranges` row ranges, into the scan's bound table; the scan then runs frozen
// (csrc/flat_collect.hip "lists beyond 128 entries")
struct CollectBigRanges {
	int ranges = 0;       // launch_collect_big_bounds: class slots per range in p.gslot [ranges][nq][128]
	int64_t rows = 0;     // rows of a range actually scanned
	float *stage = nullptr; // launch_collect_big_bounds_seed: [ranges][nq][16], the register pre-pass kernel's class maxima (ceil(k / 8) strides)
};
void launch_collect_big_bounds(const CollectPass &p, const CollectBigRanges &r);
void launch_collect_big_bounds_seed(const CollectPass &p, const CollectBigRanges &r); // (the d <= 128 store)
// counts the (truncated) stream's entries per query, takes the queries above `share` out of the coarse filter; returns how many
struct CollectDropHeavy {
	const unsigned long long *stream = nullptr;
	int64_t n = 0, nq = 0;
	int share = 0;
	int *qcount = nullptr; // [nq + 16], zeroed
	float *e2 = nullptr;
	FailList fail;
};
int launch_collect_drop_heavy(const CollectDropHeavy &h, hipStream_t st);
// thr[q] = B - 2E from the class slots as the scan left them: the final-bound filter of the bucketed finish and of filter-then-sort
void launch_collect_final_thr(const CollectPass &p, float *d_thr);
// the words the host reads after a search, into pinned memory (collect_report_kernel)
struct CollectReportSrc {
	const void *hdr = nullptr; // the control block, or null
	const int *fail_cnt = nullptr;
	const unsigned *maxnorm = nullptr;
	int *h_flags = nullptr;
	void *h_hdr = nullptr; // (may be null) the control block's header goes here
	bool with_cnt = false;
};
void launch_collect_report(const CollectReportSrc &r, hipStream_t st);

// ---- csrc/flat_collect.hip: the sorted pipeline ---------------------------------------------------------------------------------------
size_t collect_select_big_temp_bytes(int64_t ncand, int64_t nq);
// Entries the deferred sort of a search is launched with, from the candidates per query c of the index's previous search: the
// margin shrinks with the batch (the mean of nq heavy-tailed per-query counts), 17 % + 16 per query at 10 000 queries, 40 % at 64
// (round 4, first cut: 30 % + 64 per query whatever the batch -- at C3's 149 per query the sort ran over 75 % more entries than it had)
static inline int64_t collect_sort_estimate(double c, int64_t nq) {
	const double per = c * (1.15 + 2.0 / sqrt((double)std::max<int64_t>(nq, 1))) + 16.0;
	return ((int64_t)(per * (double)nq) + 65535) / 65536 * 65536;
}
size_t collect_sort_temp_bytes(int64_t ncand, int64_t nq);
size_t collect_sort_temp_bytes_est(int64_t n_est, int64_t nq);
// stream (ncand entries) -> per query the kk best exact candidates: pd1 / pi1 [nq][kk] (value, row), best first
struct CollectRescore {
	int metric = 0;
	unsigned long long *stream = nullptr, *sorted = nullptr;
	int64_t ncand = 0;
	const unsigned long long *cnt = nullptr; // != null: device-count mode -- ncand is the host's estimate, the real number min(*cnt, ncand)
	void *temp = nullptr;
	size_t temp_bytes = 0;
	int *seg = nullptr; // [2 nq] begin | end of every query's segment
	bool seg_zeroed = false;
	int64_t nq = 0;
	int kk = 0;
	// the exact stage
	const float *x = nullptr;
	FlatGeom g;
	const float *vecs = nullptr, *norms = nullptr, *qn = nullptr;
	bool per_pair = false;
	float *pd1 = nullptr;
	int32_t *pi1 = nullptr;
};
void launch_collect_rescore(const CollectRescore &r, hipStream_t st);
// A_k of the flagged inner-product queries from the exact keys of the candidate list: a query's segment of the sorted list (pitch = 0,
// seg = [2 nq] begin | end), or its bucket of the bucketed finish (pitch > 0, seg = the per-query counts)
struct CollectTieRows {
	const unsigned long long *keys = nullptr;
	const int *seg = nullptr;
	int64_t nq = 0;
	int pitch = 0;
	const int *flag_query = nullptr;
	const float *T = nullptr;
	int nf = 0, k = 0;
	int64_t *first = nullptr;
};
void launch_collect_tie_rows(const CollectTieRows &t, hipStream_t st);
void launch_stream_refilter(const CandStream &in, const float *d_thr, unsigned long long *d_out, unsigned long long *d_out_cnt, hipStream_t st);

// ---- csrc/coarse_select.hip: distance matrix + selection ------------------------------------------------------------------------------
bool coarse_select_supported(int64_t nlist, int64_t np);
// D (scratch, [nq][nlist]) <- distances; pd / pi [nq][np] <- the np nearest centroids of every query, unordered
struct CoarseSelect {
	const float *x = nullptr;
	int64_t nq = 0;
	int d = 0;
	const float *cent = nullptr;
	int sdp = 0, interleaved = 0;
	int64_t nlist = 0;
	const float *qn = nullptr, *cn = nullptr;
	int64_t np = 0;
	int is_l2 = 0;
	float *D = nullptr;
	float *pd = nullptr;
	int32_t *pi = nullptr;
	float *outD = nullptr; // (may be null) the ordered lists, labels + label_offset
	int64_t *outI = nullptr;
	int64_t label_offset = 0;
};
void launch_coarse_select(const CoarseSelect &c, hipStream_t st);

// ---- csrc/coarse_bf16.hip: the coarse quantiser as a bf16 filter + exact re-scoring inside one workgroup per 32 queries ----------------
bool coarse_bf16_supported(int d, int64_t nlist, int64_t np);
size_t coarse_bf16_cand_bytes(int64_t nq);
size_t coarse_bf16_cls_bytes(int64_t nq, int64_t nlist, int64_t np);
int coarse_bf16_slices(int64_t nq, int64_t nlist, int64_t np);
struct CoarseBf16 {
	const float *x = nullptr;
	int64_t nq = 0;
	int d = 0;
	const void *qf = nullptr; // qf / qn / e2: what launch_collect_query_prep left for these nq queries
	const float *qn = nullptr, *e2 = nullptr;
	const unsigned short *yb = nullptr; // yb / beta: the quantiser's centred bf16 store
	const float *beta = nullptr;
	const float *cent = nullptr; // the f32 rows, their pitch and layout, their norms
	int sdp = 0, interleaved = 0;
	const float *cn = nullptr;
	int64_t nlist = 0, np = 0;
	unsigned short *cand = nullptr; // workspaces: coarse_bf16_cand_bytes, [nq] ints, coarse_bf16_cls_bytes
	int *ccount = nullptr;
	float *cls = nullptr;
	float *outD = nullptr;
	int64_t *outI = nullptr;
	int64_t label_offset = 0;
	unsigned long long *stats = nullptr;
};
void launch_coarse_bf16(const CoarseBf16 &c, hipStream_t st);

// ---- csrc/ivf_collect.hip -------------------------------------------------------------------------------------------------------------
struct IvfStoreRows {
	const float *res = nullptr; // the residual rows
	int64_t nrows = 0;
	int d = 0;
	const int *list_of_blk64 = nullptr;
	unsigned short *bf = nullptr;
	float *beta = nullptr;
	unsigned *list_max_bits = nullptr; // [2 nlist]
	int64_t nlist = 0;
};
void launch_ivf_rows_to_bf16(const IvfStoreRows &r, hipStream_t st);
size_t ivf_collect_xi_bytes(int max_items);
// Work items of a list scan (128 query slots each) and what the packing kernel leaves per item slot
struct IvfItemSet {
	const void *items = nullptr;
	const int *nitems = nullptr; // on the device
	int max_items = 0;
	const int *qidx = nullptr;
	void *xi = nullptr;      // fragments: ivf_collect_xi_bytes
	float *igamma = nullptr; // [max_items][128]
	float *ie2 = nullptr;
};
// what the packing of both item sets shares; slots0: the near set's slot of every query
struct IvfPackShared {
	const float *x = nullptr;
	int d = 0;
	int64_t nq = 0;
	const int *slots0 = nullptr;
	const float *cent = nullptr;
	const int *list_of_blk64 = nullptr;
	const unsigned *list_max_bits = nullptr;
	int *qfail = nullptr;
	int64_t nlist = 0;
	unsigned *gslot = nullptr; // class slots -> neutral, control block and flag count -> 0 on the way
	int nclass = 0;
	int *ctl_hdr = nullptr, *flag_cnt = nullptr;
};
void launch_ivf_collect_pack2(int metric, const IvfPackShared &sh, const IvfItemSet &near_set, const IvfItemSet &scan_set, hipStream_t st);
// the store, the class slots and the segmenting of a list scan
struct IvfListScan {
	const unsigned short *rows_bf = nullptr;
	const float *beta = nullptr;
	unsigned *gslot = nullptr;
	int kk = 0;
	int seg_rows = 0, nseg = 0;
	int collect = 0; // 0: publish to the slots only
	const unsigned *rowmask = nullptr;
	const float *bfix = nullptr; // (may be null) frozen bounds
};
void launch_ivf_collect_scan(const IvfItemSet &it, const IvfListScan &sc, const CandStream &s, hipStream_t st);
// the final bound per query from the class slots (gslot == null: bf holds the thresholds already -- the Flat index, launch_collect_final_thr)
struct IvfFinalBound {
	const unsigned *gslot = nullptr;
	int nclass = 0, kf = 0;
	int64_t nq = 0;
	float *bf = nullptr;
};
// final-bound filter between the scan and the exact stage: entries whose s + E is below the bound the scan ended with are dropped
void launch_ivf_refilter(const CandStream &in, const IvfFinalBound &fb, unsigned long long *d_out, unsigned long long *d_out_cnt, hipStream_t st);
size_t ivf_bucket_units_bytes(int64_t cap_entries);
unsigned ivf_bucket_scatter_blocks(int64_t cap_entries);
// final bound + the survivors into their queries' row buckets; launch_ivf_bucket_finish re-scores them (IvfBucketFinish::brow)
struct IvfRowBuckets {
	unsigned *brow = nullptr;   // [nq][bpitch] padded row numbers
	unsigned *bcount = nullptr; // [nq] every survivor counted, also those past the pitch
	int bpitch = 0;
	int *kept_blk = nullptr; // per-workgroup survivor counts: ivf_bucket_scatter_blocks of them
	unsigned long long *units = nullptr; // ivf_bucket_units_bytes
	unsigned *unit_cnt = nullptr;
};
void launch_ivf_bucket_scatter(const CandStream &in, const IvfFinalBound &fb, const IvfRowBuckets &b, hipStream_t st);
// stream or row buckets -> exact values into per-query key buckets -> the kk best -> the search's output (ivf_bucket_select_kernel)
struct IvfBucketFinish {
	int metric = 0;
	int64_t nq = 0;
	// the source: the scan's candidate stream (ncand = its capacity or the host's count; the real number is min(*cnt, ncand)) ...
	const unsigned long long *strm = nullptr;
	int64_t ncand = 0;
	const unsigned long long *cnt = nullptr;
	// ... or (brow != null) the rows in their queries' buckets already (launch_ivf_bucket_scatter), with its work units
	const unsigned *brow = nullptr;
	const unsigned long long *units = nullptr;
	const unsigned *unit_cnt = nullptr;
	// the exact stage: queries, the row store with its pitch, permutation and interleaving
	const float *x = nullptr;
	int d = 0;
	const float *rows = nullptr;
	int dp = 0;
	const int *perm = nullptr;
	int rows_interleaved = 0;
	const IvfFlatArith *fa = nullptr; // != null: the Flat index's arithmetic -- the lists come out in FAISS's Flat L2 order
	// the key buckets [nq][bpitch] and their counts [nq] (zeroed)
	unsigned long long *bucket = nullptr;
	unsigned *bcount = nullptr;
	int bpitch = 0;
	// the selection: pd / pi [nq][kk], the pure list; labels through rowids (null: the keys' low words as they are), then through
	// idmap if given, or + label_offset
	int kk = 0;
	float *pd = nullptr;
	int64_t *pi = nullptr;
	const int64_t *rowids = nullptr, *idmap = nullptr;
	int64_t label_offset = 0;
	// the final print of the IVF exact-tie wrapper (D != null): D / I [nq][k], k < kk, FAISS's print order + the boundary-tie flags
	int k = 0;
	float *D = nullptr;
	int64_t *I = nullptr;
	const int64_t *fin_rowids = nullptr, *fin_idmap = nullptr;
	int *flag = nullptr; // [1 + nq] count | queries
	const IpFlatEmit *ipf = nullptr; // the Flat index's inner-product output
	// per-query fail flags -> fail.queries[(*fail.count)++]
	int *qfail = nullptr;
	FailList fail;
	unsigned long long *stats = nullptr; // [0] sum of the bucket counts, [1] the largest
	bool reset = false; // leave bcount[q] and qfail[q] zero for the next search
	// (may be null) per-workgroup survivor counts of the scatter kernel; their sum goes to kept_out
	const int *kept_blk = nullptr;
	int nkept_blk = 0;
	unsigned long long *kept_out = nullptr;
};
void launch_ivf_bucket_finish(const IvfBucketFinish &f, hipStream_t st);
// probed lists that provably hold none of a query's k nearest rows -> -1 in out (ivf_probe_prune_kernel); np <= 256
struct IvfProbePrune {
	const float *x = nullptr;
	int64_t nq = 0;
	int d = 0;
	const float *cD = nullptr; // [nq][np] computed coarse distances, ascending
	const int64_t *cI = nullptr;
	int np = 0, k = 0;
	const float *cn = nullptr; // [nlist] ||c||^2
	const unsigned *list_max = nullptr;
	const int64_t *list_off = nullptr; // [nlist + 1]
	int64_t *out = nullptr;            // [nq][np]
	int *kept = nullptr;               // [nq] probes kept (statistics), may be null
};
void launch_ivf_probe_prune(const IvfProbePrune &p, hipStream_t st);
// Flat shadow: is the probed set provably enough?  (csrc/ivf_collect.hip ivf_shadow_verify_kernel, whose argument this is)
struct IvfShadowVerifyArgs {
	const float *cmat;     // [nq][nlist] computed coarse distances
	const float *cD;       // [nq][np] the probed lists' distances, ascending
	const long long *cI;   // [nq][np] the probed lists
	int nlist, np, d, k;
	const float *qn;       // [nq] ||x||^2
	const float *cn;       // [nlist] ||c||^2
	const unsigned *list_max; // [nlist] largest ||y - c||^2 of every list (bit pattern)
	const long long *lb, *le; // padded row range of every list (empty: lb == le)
	const float *D;        // [nq][k] the results
	const long long *I;
	const unsigned *ymax_bits; // the Flat index's largest ||y||^2 (bit pattern)
	int *fail_cnt;
	int *fail_q;
};
void launch_ivf_shadow_verify(const IvfShadowVerifyArgs &a, int64_t nq, hipStream_t st);
size_t ivf_rowmask_bytes(int64_t nrows_mf);
struct IvfRowmask {
	const int64_t *rowids_mf = nullptr;
	const int *perm = nullptr;
	const int64_t *idmap = nullptr;
	int64_t nrows_mf = 0;
	void *mask = nullptr; // ivf_rowmask_bytes
};
void launch_ivf_rowmask(SelectorDev sel, const IvfRowmask &m, hipStream_t st);
void launch_collect_flat_items(void *d_items, int *d_nitems, int *d_qidx, int64_t nq, int64_t n, hipStream_t st);

} // namespace mvs
