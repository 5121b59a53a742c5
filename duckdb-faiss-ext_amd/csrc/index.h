// csrc/index.h -- device-native index classes behind the C ABI (include/mi355_faiss.h).
#pragma once
#include "common.h"
#include "dev_mem.h"

#include "../../include/mi355_faiss.h"

#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace mvs {

// ring of pinned host buffers: the caller's rows are copied here so add()/search() can return /
// overlap while hipMemcpyAsync drains the slot (SURVEY.md 8f-1 ingest staging)
struct PinnedRing {
	static constexpr int NB = 4;
	static constexpr size_t SLOT_BYTES = 8u << 20;
	void *buf[NB] = {nullptr, nullptr, nullptr, nullptr};
	size_t cap[NB] = {0, 0, 0, 0};
	hipEvent_t ev[NB] = {nullptr, nullptr, nullptr, nullptr};
	int next = 0;
	int acquire(size_t bytes);
	void release(int slot, hipStream_t st);
	void drop_events();
	~PinnedRing();
};

// the ids a call's scan will test against its selector, entry i of n: raw = d_ids ? d_ids[i] : offset + i (an IVF kind's stored ids, or the
// rows), and the tested id is d_map ? d_map[raw] : raw (the id map a wrapper passed down) -- what every scan kernel computes before its
// sel_member call.  Taken after staged rows and ids are flushed.  Only MVS_SEL_PROGRAM reads it (csrc/selector_lower.hip)
struct IdDomain {
	const int64_t *d_ids = nullptr;
	int64_t offset = 0, n = 0;
	const int64_t *d_map = nullptr;
	static IdDomain rows(int64_t offset, int64_t n, const int64_t *d_map = nullptr) { // (the offset is the kind's label offset where the scan adds it; none under a map)
		return IdDomain {nullptr, d_map ? 0 : offset, n, d_map};
	}
	static IdDomain ids(const int64_t *d_ids, int64_t n, const int64_t *d_map = nullptr) {
		return IdDomain {d_ids, 0, n, d_map};
	}
};
// what a handle keeps about selector programs (include/mi355_faiss.h "selector programs"): option sel_bitmap_cap_bytes, statistics
// sel_lowered / sel_admitted.  The C ABI's entry points that take a selector name theirs for the thread while the call runs
// (SelectorCallScope, which also refuses a malformed program before anything is touched); SelectorHolder::upload reads and fills it
struct SelectorCall {
	int64_t cap_bytes = 0; // 0: automatic
	int lowered = 0;       // 0 none | 1 bitmap | 2 batch
	int64_t admitted = 0;
};
extern thread_local SelectorCall *t_selector_call;
struct SelectorCallScope {
	SelectorCall *prev;
	SelectorCallScope(SelectorCall &c, const mvs_search_params *p);
	~SelectorCallScope();
	SelectorCallScope(const SelectorCallScope &) = delete;
	SelectorCallScope &operator=(const SelectorCallScope &) = delete;
};

struct SelectorHolder {
	DevBuf buf; // what the returned SelectorDev points to: the bitmap, or the ascending ids
	std::vector<int64_t> sorted;
	DevBuf prog, bits, ids, temp, stats; // MVS_SEL_PROGRAM: packed program, admitted bits, compacted ids, the sort's scratch, (count, min, max)
	// plain kinds ignore `dom`; a program is evaluated over it and lowered to a plain selector (synchronises `st` once)
	SelectorDev upload(const mvs_search_params *p, const IdDomain &dom, hipStream_t st);
	void release(); // the index leaves its device: every buffer goes
private:
	SelectorDev upload_program(const mvs_search_params *p, const IdDomain &dom, hipStream_t st);
};

// Host-side image of an index: what faiss::write_index stores (impl/index_write.cpp).  Used by index_io.hip and by
// cross-device clones (faiss::gpu::index_cpu_to_gpu), both of which go through host memory.
// one transform of an IndexPreTransform chain (csrc/pretransform.hip), as faiss::write_VectorTransform stores it
struct HostTransform {
	int type = 0; // MVS_VT_LINEAR | MVS_VT_PCA | MVS_VT_NORM
	int d_in = 0, d_out = 0;
	bool have_bias = false, is_trained = false;
	std::vector<float> A, b; // LinearTransform: [d_out][d_in], [d_out]
	// PCAMatrix: kept for writing the transform back as "PcAm"
	float eigen_power = 0.f, epsilon = 0.f;
	bool random_rotation = false;
	int32_t balanced_bins = 0;
	std::vector<float> mean, eigenvalues, PCAMat;
	float norm = 2.f; // NormalizationTransform
};

struct HostIndex {
	int kind = 0, d = 0, metric = 0;
	float metric_arg = 0.f;
	int64_t ntotal = 0;
	bool is_trained = true;
	std::vector<float> rows;       // Flat: [ntotal][d]
	std::unique_ptr<HostIndex> sub; // IDMap: wrapped index; IVF: quantizer; HNSW: storage (a Flat image)
	std::vector<int64_t> ids;      // IDMap: id_map
	bool idmap2 = false;
	int64_t nlist = 0, nprobe = 1; // IVF
	std::vector<std::vector<int64_t>> list_ids;
	std::vector<std::vector<float>> list_codes; // per list [n][d]
	// HNSW (struct HNSW fields in FAISS's order)
	std::vector<double> assign_probas;
	std::vector<int32_t> cum_nneighbor_per_level, levels, neighbors;
	std::vector<uint64_t> offsets;
	int32_t entry_point = -1;
	int max_level = -1, efConstruction = 40, efSearch = 16;
	// PQ (csrc/pq.hip): ProductQuantizer::M, centroids [M][256][d / M], codes [ntotal][M]
	int pq_M = 0;
	std::vector<float> pq_centroids;
	std::vector<uint8_t> pq_codes;
	// IVFPQ (csrc/ivfpq.hip): nlist, nprobe, sub (the quantizer), list_ids, pq_M, pq_centroids as above; per list [n][pq_M] code bytes
	std::vector<std::vector<uint8_t>> list_bytes;
	// SQ8 / IVF<n>,SQ8 (csrc/sq.hip): ScalarQuantizer::trained = vmin [d] | vdiff [d]; SQ8: codes [ntotal][d]; the IVF kind: nlist, nprobe,
	// sub (the quantizer), list_ids, per list [n][d] code bytes in list_bytes
	std::vector<float> sq_trained;
	bool sq_has_range = false; // the range is present (an index can hold it before its centroids: not trained yet)
	std::vector<uint8_t> sq_codes;
	// Refine (csrc/refine.hip): sub (the base index), sub2 (the refine store, a Flat image), k_factor
	std::unique_ptr<HostIndex> sub2;
	float k_factor = 1.f;
	// PreTransform (csrc/pretransform.hip): the chain, then sub (the index at the chain's output dimension); d is the chain's input dimension
	std::vector<HostTransform> chain;
};

// indexes constructed while one of these is alive (same thread) live on `dev` instead of MVS_DEVICE
struct CtorDevice {
	int prev;
	explicit CtorDevice(int dev);
	~CtorDevice();
};

// ---- one pass of the Flat search (DESIGN.md 3.1 "Host driver"): FlatIndex::search_flat builds one for the caller's batch, the tie wrapper
// the k + 1 one, a re-run of unproven queries its own.  The driver's functions take it by const reference: no member says what a pass is for.
struct FlatSearchRequest {
	int64_t nq;
	const float *d_x;
	int64_t k_user, kk; // entries printed per query / selected per query: k_user + 1 under the inner-product tie detection
	float *D;
	int64_t *I;
	const mvs_search_params *params;
	const int64_t *d_idmap;
	const int64_t *out_map; // label translation of the merge: out_map[row], or row + out_off
	int64_t out_off;
	const TieFlags *flags; // where the merge records the queries tied at the k-th score (null: no tie detection)
	hipStream_t st;        // the caller's stream
	bool pair_branch = false; // FAISS's per-pair branch, decided by the BATCH this pass belongs to (its nq < 20): a re-run inherits it
	bool exact_only = false;  // the re-run of queries a filter's proof rejected: no filter may take the pass
	bool no_shadow = false;   // the shadow's own re-run: the shadow may neither take the pass nor be marked wanted by it
	bool quiet = false;       // a re-run leaves no trace: no kernel timing, kinfo as the outer pass left it
	bool has_sel() const {
		return params && params->sel_kind != MVS_SEL_NONE;
	}
};
// what an exact branch of the Flat search launched (FlatIndex::finish_exact): 256 threads per workgroup, one partial list per row range
struct ExactLaunch {
	SelectorDev sel;
	int nparts, grid, lds_bytes;
	const char *name;
	double flops, bytes;
};

// ---- one pass of the Flat coarse filter (csrc/flat_coarse.hip): what FlatIndex::search_prefilter_pass asks of
// FlatIndex::collect_candidates and what comes back.  Nothing of a pass lives in the index between two searches.
struct CollectRequest {
	int64_t nq;
	const float *d_x;
	int kk; // entries selected per query
	int kf; // kf <= kk: the k the FILTER works with (class slots, bound rank) -- see search_prefilter_pass
	const mvs_search_params *params;
	const int64_t *d_idmap;
	int *fail_cnt, *fail_q; // the queries whose bound is not finite (and the heavy ones of an overflow) join this list
	// nothing waits for the candidate count between the scan and the re-scoring (device-count mode); the count reaches the pinned report
	// asynchronously and the caller checks it against CollectResult::deferred_cap after ITS stream synchronisation -- on an overflow it
	// runs the search again with defer_count = false (the synchronous overflow handling)
	bool defer_count;
	// the final lists, where collect_candidates may write them itself (D == nullptr: it must not): L2 as they are, inner product with
	// the boundary-tie flags of the search (or null) and kout entries printed per query (the selection carries kk >= kout)
	float *D;
	int64_t *I;
	const int64_t *map;
	int64_t off;
	const TieFlags *flags;
	int kout;
	hipStream_t st;
};
// Where FlatIndex::resolve_ip_ties finds the rows tied at a flagged query's boundary score after a coarse-filter pass -- every row at or
// above that score is a candidate, so the database is not scanned again: the re-scored candidate list, or the bucketed finish's buckets
struct TieSource {
	const unsigned long long *sorted = nullptr; // the candidate list grouped by query (in ws_stream; segments in the control block) ...
	const unsigned long long *bucket = nullptr; // ... or every survivor's exact key in its query's bucket, [nq][bpitch] (lists below 100 entries only),
	const unsigned *bcount = nullptr;           // the buckets' fill
	int bpitch = 0;
};
struct CollectResult {
	bool ok = false; // false: the candidate stream overflowed, or the shape is not served (the caller falls back)
	float *pd1 = nullptr; // [nq][kk] the kk best exact candidates per query (null when emitted)
	int32_t *pi1 = nullptr;
	bool emitted = false;     // the final lists are written (the caller skips its emission)
	bool filtered = false;    // the stream was compacted with the final-bound filter (wide stores): CollectCtl::kept counts the survivors
	bool report_cnt = false;  // the scan's entry count (and the control block's header) still has to reach the host: launch_collect_report does it
	int64_t deferred_cap = 0; // deferred count mode: entries the sort / the stream covered; 0: the pass was synchronous
	TieSource tie;
};
// ---- range search (csrc/range_search.hip; include/mi355_faiss.h "range search") ----------------------------------------------
// what faiss::RangeSearchResult carries, in host memory: query q's hits are entries [lims[q], lims[q + 1])
struct RangeResult {
	std::vector<int64_t> lims; // [nq + 1]
	std::vector<float> distances;
	std::vector<int64_t> labels;
	void clear(int64_t nq); // nq + 1 zeros, no entries
};
// what an index keeps between range searches: the hit stream and the sort's buffers (grow-only), option and statistic
struct RangeWork {
	DevBuf keys, vals, skeys, svals, temp, ctl, items;
	int64_t stream_cap = 0; // option range_stream_cap: entries of the first attempt's stream (0: automatic)
	int64_t rescans = 0;    // statistic range_rescans: scans repeated because the stream was too small
	void release() { // the index leaves its device (FlatIndex::to_device): every buffer goes, option and statistic stay
		DevBuf *const all[] = {&keys, &vals, &skeys, &svals, &temp, &ctl, &items};
		static_assert(sizeof all / sizeof *all * sizeof(DevBuf) + 2 * sizeof(int64_t) == sizeof(RangeWork), "a buffer of RangeWork is missing from release()");
		for (DevBuf *b : all)
			b->release();
	}
};
// one scan of one chunk of queries against one row store
struct RangeScan {
	int metric;
	int64_t nq;
	const float *xq; // [nq][dp], zero padded (the MFMA kernel: to whole blocks of 128 queries)
	const float *xn; // [nq] squared query norms (formula)
	const float *rows, *norms;
	int64_t nrows;
	int dp;
	bool interleaved, formula; // FlatGeom::pair_interleaved; L2 as (xn + yn) - 2 ip instead of the per-pair chain
	float radius;
	SelectorDev sel;
	const int64_t *idmap_sel; // the selector tests idmap_sel[stored id]
	unsigned long long *keys, *vals, *cnt; // the stream (set by range_collect)
	int64_t cap;
};
bool range_mfma_supported(const FlatGeom &g);
void launch_range_flat(const RangeScan &s, bool mfma, int *grid_out, hipStream_t st);
size_t range_ivf_item_bytes(int64_t npairs);
// d_coarse [nq][np] probed lists in rank order (-1: none), d_list_off [nlist + 1] their bounds in the list-sorted store
void launch_range_ivf(const RangeScan &s, const int64_t *d_coarse, int np, const int64_t *d_list_off, const int64_t *d_rowids, void *d_items,
                      hipStream_t st);
// queries [q0, q0 + s.nq) of the call: `scan` fills the stream (a second time when it was too small), then sort by (query, ordinal),
// lims, labels (d_rowids[position] if given, then d_idmap_out[.] or + label_offset) and the copies behind `out`
void range_collect(RangeWork &w, RangeScan s, const std::function<void(const RangeScan &)> &scan, int64_t q0, const int64_t *d_rowids,
                   const int64_t *d_idmap_out, int64_t label_offset, RangeResult &out, hipStream_t st);

// ---- remove_ids (csrc/remove_ids.hip; include/mi355_faiss.h "remove_ids") --------------------------------------------------------
// which rows of a store go, on the device: flags[r] = 1 for a survivor (entry n is 0), dest = their exclusive scan, so dest[r] is the
// survivor's new row and dest[n] the survivor count.  Rows are arrival positions (Flat, PQ, SQ8) or stored ids (an IVF kind under IDMap)
struct RemoveMarks {
	DevBuf flags, dest, temp; // unsigned [n + 1] each; the scan's scratch
	int64_t n = 0, nkeep = 0;
};
void check_remove_selector(const mvs_search_params *sel); // MVS_SEL_BITMAP | MVS_SEL_BATCH with host data or a well-formed MVS_SEL_PROGRAM, or it throws
// one thread per row: a member of `sel` (tested on d_idmap[r], or on label_offset + r) goes; then the scan.  Synchronises `st`; returns nkeep
int64_t remove_mark(RemoveMarks &m, SelectorDev sel, const int64_t *d_idmap, int64_t label_offset, int64_t n, hipStream_t st);
int64_t remove_marks_from_host(RemoveMarks &m, const uint8_t *keep, int64_t n, hipStream_t st); // the same from host flags
// stable compaction: rows of `pitch` bytes (a multiple of 16) moved as uint4; the int64 id map; the Flat f32 store with its norms -- a
// survivor whose new row number differs in bit 4 has every group of four floats re-permuted on the way (FlatGeom::pair_interleaved)
void launch_remove_compact_rows(const void *d_src, int pitch, const RemoveMarks &m, void *d_dst, hipStream_t st);
void launch_remove_compact_i64(const int64_t *d_src, const RemoveMarks &m, int64_t *d_dst, hipStream_t st);
void launch_remove_compact_flat(const FlatGeom &g, const float *d_vecs, const float *d_norms, const RemoveMarks &m, float *d_dst, float *d_dst_norms,
                                hipStream_t st);
// dst row i = src row perm[i], rows of `pitch` bytes (a multiple of 16): the IVF kinds' arrival-order stores by the host plan's permutation
void launch_remove_gather_rows(const void *d_src, const int *d_perm, int64_t n, int pitch, void *d_dst, hipStream_t st);
// the host side of an IVF kind's removal (csrc/remove_plan.h): membership of the stored ids (of d_idmap[stored id] under IDMap, with the
// renumbering and, in `marks`, the flags by stored id for the wrapper), the per-list swap loops and the new list-major arrival order.
// false: nothing goes.  Otherwise `plan` holds the new directory and perm [nkeep], each new arrival position's old one: the caller
// adopts it (ListDirectory::adopt, csrc/list_directory.h) once its store is gathered
struct IvfRemovePlan;
struct ListDirectory;
bool ivf_remove_plan_host(const ListDirectory &dir, const mvs_search_params *sel, const int64_t *d_idmap, RemoveMarks *marks, IvfRemovePlan &plan,
                          hipStream_t st);

// ---- merge_from and copy_subset_to (csrc/merge.hip; include/mi355_faiss.h "merge_from and copy_subset_to") ------------
// Flat rows [src_row0, src_row0 + n) of one store -> rows [dst_row0, ...) of another of the same geometry, with their norms.  In the
// pair-interleaved layout a row whose new number differs in bit 4 has the halves of every group of four floats swapped on the way
void launch_merge_flat_rows(const FlatGeom &g, const float *d_src, const float *d_src_norms, int64_t src_row0, int64_t n, float *d_dst,
                            float *d_dst_norms, int64_t dst_row0, hipStream_t st);
// rows of `pitch` bytes (a multiple of 16): dst row dst_row0 + i = src row d_pos[i], or src row i without d_pos (the contiguous path)
void launch_merge_append_rows(const void *d_src, const int64_t *d_pos, int64_t n, int pitch, void *d_dst, int64_t dst_row0, hipStream_t st);
void launch_merge_append_ids(const int64_t *d_src, int64_t n, int64_t add_id, int64_t *d_dst, hipStream_t st); // dst[i] = src[i] + add_id
bool merge_dev_equal(const void *d_a, const void *d_b, size_t bytes, hipStream_t st); // byte for byte, compared on the device; synchronises `st`
class IndexBase;
struct CoarseSide;
// what every kind's check_compatible_for_merge begins with: other is not this, neither is sharded, the same kind, d, metric and device
void merge_check_common(IndexBase &a, IndexBase &b);
// ... and what a kind with inverted lists adds: nlist, both trained, the coarse centroids bit for bit
void merge_check_coarse(IndexBase &a, CoarseSide &ca, IndexBase &b, CoarseSide &cb);
[[noreturn]] void merge_refuse(const char *fmt, ...); // "check_compatible_for_merge: <the first difference>"
[[noreturn]] void merge_refuse_add_id();              // Flat, PQ, SQ8 with add_id != 0: FAISS's "cannot set ids in FlatCodes index"
void merge_check_subset_type(int subset_type, int64_t a1); // copy_subset_to: types 0, 1 (a1 > 0), 2
// MVS_MERGE_PROFILE=1: where a merge's time goes, on stderr -- "mergeprofile\t<kind> <phase>: <ms>" (tools/merge_bench.py).  A lap
// synchronises `st` first, so that a phase's device work is counted where it was enqueued
struct MergeLaps {
	const char *kind;
	const bool on;
	double t_prev_ms;
	explicit MergeLaps(const char *kind);
	void lap(const char *what, hipStream_t st);
};

// ---- reconstruct (csrc/reconstruct.hip; include/mi355_faiss.h "reconstruct") ------------------------------------------
// The device table of a kind that stores ids: (key, position) sorted by key, equal keys by ascending position, so the LAST entry of a run is
// the row added last.  Built on first use; whatever changes the ids or the order of the rows drops it
struct ReconTable {
	DevBuf keys, pos, assign; // int64 [n] ascending | unsigned [n] | int [n]: the list of the row at a position (coded IVF kinds; -1: none)
	int64_t n = -1;           // -1: not built
	bool valid() const {
		return n >= 0;
	}
	void drop() {
		keys.release(), pos.release(), assign.release();
		n = -1;
	}
};
// ids by position come from the host (h_ids; an IVF kind's ids_h) or are on the device already (d_ids; IDMap's id map); h_assign may be null
void recon_table_build(ReconTable &t, const int64_t *h_ids, const int64_t *d_ids, const int32_t *h_assign, int64_t n, hipStream_t st);
// one step of key -> row: a table (upper bound - 1 of the key), or without one the range check of key - off against [0, n)
struct ReconStage {
	const long long *keys;
	const unsigned *pos;
	long long n, off;
};
enum { RECON_F32 = 0, RECON_SQ8 = 1, RECON_PQ = 2 };
// where a kind's rows live and how a row becomes d f32 values: what IndexBase::recon_source fills for the gather / decode kernels
struct ReconSource {
	int mode = RECON_F32;
	const void *rows = nullptr; // f32 rows or code rows, by position
	long long pitch = 0;        // bytes between rows
	long long nrows = 0;
	int interleaved = 0;                            // RECON_F32: FlatGeom::pair_interleaved
	const float *sq_a = nullptr, *sq_s = nullptr;   // RECON_SQ8: dec(c, k) = a[k] + (float)c s[k]
	const float *cb = nullptr;                      // RECON_PQ: codebooks [M][256][dsub]
	int M = 0, dsub = 0;
	const float *cent = nullptr; // the coded IVF kinds: centroids [nlist][d], added to the decoded residual of a row of list assign[position]
	const int *assign = nullptr;
	int nstage = 0; // key -> position, outermost first (IDMap's map, then the wrapped kind's)
	ReconStage stage[2] {};
	hipStream_t owners[4] {}; // the streams that own the stores read: a device-resident call makes them wait for the caller's stream
	int nowners = 0;
	void push_stage(const ReconStage &s) {
		stage[nstage++] = s;
	}
	void own(hipStream_t s) {
		if (nowners < 4)
			owners[nowners++] = s;
	}
};
enum { RECON_STRICT = 0, RECON_PAD = 1, RECON_SKIP = 2, RECON_PAD_UNCHECKED = 3 };

struct CollectPlan; // csrc/flat_coarse.hip
struct CollectWork;
struct PrefilterRoute;
struct CollectCtl; // csrc/flat_collect.h
struct CollectReport;

class IndexBase {
public:
	int kind, d, metric;
	int64_t ntotal = 0;
	bool is_trained = true;
	int device = 0;
	hipStream_t stream = nullptr;
	int64_t label_offset = 0;
	float metric_arg = 0.f; // faiss::Index::metric_arg (Lp exponent); the glue leaves it at 0
	// base of a RefineIndex (csrc/refine.hip), in the manner of FlatIndex::raw_rows: an id map passed to search_mapped feeds the selector
	// only, labels stay raw (the stored id, which there is the row number of the refine store).  Honoured by the four scanning kinds
	// (csrc/pq.hip, csrc/coded_lists.hip) in the arguments of their emit kernels; no kernel reads it
	bool raw_labels = false;
	// wrappers (IDMap, Refine) re-read is_trained from what they wrap: codebooks / centroids / ranges set through a borrowed handle
	// of the wrapped index (mvs_index_refine_base) train it behind the wrapper's back
	virtual void refresh_trained() {
	}
	mvs_kernel_info kinfo {};
	void set_kinfo(const char *name, double flops, double bytes, int grid, int block, int lds_bytes, int nsplit);

	IndexBase(int kind, int d, int metric);
	virtual ~IndexBase();
	void use_device() const;
	Tuning tune_;                                  // this index's tuning knobs (csrc/common.h); current for the thread after use_device()
	bool set_tuning(const char *key, int64_t v); // the option keys that are tuning knobs (csrc/index.hip)
	// a copy / shard set / shadow of an index keeps its knobs (they reverted to the defaults silently); wrappers pass it on
	virtual void adopt_tuning(const Tuning &t) {
		tune_ = t;
	}

	// faiss::Index virtuals the glue calls (src/faiss_extension.cpp:396,510,512,583,607,609,631)
	virtual void train(int64_t n, const float *x);
	virtual void add(int64_t n, const float *x) = 0;
	virtual void add_with_ids(int64_t n, const float *x, const int64_t *ids);
	virtual void search(int64_t nq, const float *x, int64_t k, float *D, int64_t *I, const mvs_search_params *params);
	// device-resident variants
	virtual void add_device(int64_t n, const float *d_x, hipStream_t st) = 0;
	virtual void add_with_ids_device(int64_t n, const float *d_x, const int64_t *d_ids, hipStream_t st);
	virtual void search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I,
	                           const mvs_search_params *params, hipStream_t st) = 0;
	// search on behalf of an IndexIDMap wrapper: selector tests d_idmap[internal], labels = d_idmap[internal]
	virtual void search_mapped(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I,
	                           const mvs_search_params *params, const int64_t *d_idmap, hipStream_t st) = 0;
	// faiss::Index::range_search: "range search not implemented" unless the kind serves it (Flat, IVF<n>,Flat, IDMap over them).
	// range_search stages the host queries and calls range_search_mapped on `stream`; d_idmap as for search_mapped
	virtual void range_search(int64_t nq, const float *x, float radius, const mvs_search_params *params, RangeResult &out);
	virtual void range_search_mapped(int64_t nq, const float *d_x, float radius, const mvs_search_params *params, const int64_t *d_idmap,
	                                 RangeResult &out, hipStream_t st);
	// IVF row shard of a ShardedIndex: for the flagged queries of the LAST search (d_flag = {count, queries...}; the coarse assignment
	// of that search is still in place) this shard's first k rows not worse than T[f] in arrival order -- value, stored id, probe
	// rank, -1 padded (csrc/ivf_ties.hip EMIT mode)
	// faiss::Index::remove_ids: the rows whose id is a member of the selector go; returns their number.  "remove_ids not implemented for
	// this type of index" unless the kind serves it (Flat, PQ, SQ8, the IVF kinds, IDMap over them).  On behalf of an IndexIDMap wrapper
	// (d_idmap given): the selector tests d_idmap[row] (an IVF kind: d_idmap[stored id], and the survivors' stored ids are renumbered) and
	// `marks` receives what went, for the wrapper's id map
	virtual int64_t remove_ids(const mvs_search_params *sel, const int64_t *d_idmap = nullptr, RemoveMarks *marks = nullptr);
	// faiss::Index::merge_from, check_compatible_for_merge and faiss::IndexIVF::copy_subset_to (csrc/merge.hip; include/mi355_faiss.h
	// "merge_from and copy_subset_to").  The base refuses with FAISS's texts; Flat, PQ, SQ8, the IVF kinds and IDMap over them
	// override the first two, the bare IVF kinds the third.  check_compatible_for_merge throws the first difference and changes nothing;
	// merge_from calls it, then allocates, then moves the rows on the device and empties `other`
	virtual void check_compatible_for_merge(IndexBase &other);
	virtual void merge_from(IndexBase &other, int64_t add_id);
	virtual void copy_subset_to(IndexBase &other, int subset_type, int64_t a1, int64_t a2);
	// faiss::Index::reconstruct and its kin (include/mi355_faiss.h "reconstruct").  A kind that serves them says where its rows live and how
	// a key names one (on `st`: staged rows are flushed, the lookup table is built if need be); the base refuses with FAISS's text.  The
	// entry points below are csrc/reconstruct.hip's and the same for every kind
	virtual void recon_source(ReconSource &src, hipStream_t st);
	void reconstruct_batch(int64_t n, const int64_t *keys, float *out, int policy = RECON_STRICT);
	void reconstruct_n(int64_t i0, int64_t ni, float *out);
	void reconstruct_batch_device(int64_t n, const int64_t *d_keys, float *d_out, hipStream_t st);
	void search_and_reconstruct(int64_t nq, const float *x, int64_t k, float *D, int64_t *I, float *recons, const mvs_search_params *params);
	void search_and_reconstruct_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, float *d_recons,
	                                   const mvs_search_params *params, hipStream_t st);
	int recon_last_pq_lds = -1; // statistic recon_pq_lds: the last PQ decode read its codebooks from LDS (1) or through L2 (0)
	virtual void tie_emit(const int *d_flag, int nf, const float *d_x, const float *d_T, int64_t k, const mvs_search_params *params,
	                      const int64_t *d_idmap_sel, float *d_v, int64_t *d_id, int *d_p, hipStream_t st);
	// an IVF index as the internal clustering of a Flat L2 index (csrc/ivf.hip flat_shadow_search).  0: run; 1: this call's shape is
	// not served (the caller takes its normal path for the batch, the shadow stays); 2: this DATA is not served (stream / bucket limits)
	virtual int flat_shadow_search(int64_t, const float *, int64_t, const float *, float *, int64_t *, const int64_t *, int64_t,
	                               const unsigned *, int *, int *, int, hipStream_t) {
		return 1;
	}
	virtual int64_t flat_shadow_max_queries(int) { // queries one flat_shadow_search call takes (distance matrix, pair count)
		return 0;
	}
	virtual size_t device_bytes() const { // HBM held by the index's row stores (approximate; mvs_index_shadow_stats)
		return 0;
	}
	virtual void to_device(int new_device) = 0;
	virtual IndexBase *clone(int on_device) = 0; // deep copy living on `on_device`
	virtual void to_host(HostIndex &out) = 0;    // host image (write_index, cross-device clone)
	virtual void set_label_offset(int64_t off) {
		label_offset = off;
	}
	virtual const float *last_batch_ptr() const { // IVF: the device pointer of the batch whose coarse assignment the index still holds (tie_emit)
		return nullptr;
	}
	virtual bool named_stat(const char *, int64_t *) { // index-specific counters of mvs_index_get_stat (HNSW: hnsw_build_distances | hnsw_build_shortcuts)
		return false;
	}
	virtual bool probe_stats(int64_t *, int64_t *, int64_t *, int64_t *) { // IVF: (query, list) pairs of the last search / of those, scanned (mvs_index_ivf_probe_stats)
		return false;
	}
	virtual bool collect_stats(int64_t *, int64_t *, int64_t *) { // coarse-filter census of an IVF index (mvs_index_collect_stats)
		return false;
	}
	virtual bool set_option(const char *, int64_t) {
		return false;
	}

	// HIP-event timing of the dominant kernel (bench.py roofline)
	virtual void set_timing(bool on) {
		timing_enabled = on;
	}
	virtual void resolve_timing(int *count, double *total_ms) {
		resolve_kernel_timing(count, total_ms);
	}

protected:
	PinnedRing pinned;
	DevBuf ws_hx, ws_hD, ws_hI;
	DevBuf ws_rkeys, ws_rpos, ws_rout, ws_rmiss; // reconstruct: staged keys, resolved positions, staged rows, the first missing batch index
	// keys [n] (null: i0, i0 + 1, ...) -> rows at d_out, on `st`; d_miss: one word, the smallest batch index whose key names no row
	void recon_run(const ReconSource &src, int64_t n, const int64_t *d_keys, int64_t i0, float *d_out, int policy, unsigned *d_miss, hipStream_t st);
	void recon_workspaces(int64_t nkeys, size_t out_bytes);
	void recon_host(const ReconSource &src, int64_t n, const int64_t *keys, int64_t i0, float *out, int policy); // keys null: i0, i0 + 1, ...
	[[noreturn]] void recon_throw_missing(const ReconSource &src, int64_t key) const;
	bool timing_enabled = false;
	std::vector<std::pair<hipEvent_t, hipEvent_t>> timing_events;
	int timing_count = 0;
	double timing_total_ms = 0;
	// placement: the index's stream, pinned staging and the seven workspaces above leave `device` for new_device (the caller has synchronised
	// and freed its own device memory; `device` is current on entry, new_device on return)
	void move_stream(int new_device);
	const float *stage_queries(int64_t nq, const float *x); // host queries -> ws_hx through pinned staging, on `stream`
	void begin_kernel_timing(hipStream_t st);
	void end_kernel_timing(hipStream_t st);
	// A search inside a search (the queries a filter could not prove, run again on the exact kernels) leaves no trace: no kernel timing
	// while it lives, kinfo as the outer search left it afterwards -- on every exit
	struct QuietScope {
		IndexBase &ix;
		const bool timing;
		const mvs_kernel_info keep;
		explicit QuietScope(IndexBase &i) : ix(i), timing(i.timing_enabled), keep(i.kinfo) {
			ix.timing_enabled = false;
		}
		~QuietScope() {
			ix.timing_enabled = timing, ix.kinfo = keep;
		}
	};
	void resolve_kernel_timing(int *count, double *total_ms);
};

// Every device workspace a FlatIndex keeps between calls, and nothing else: a base of FlatIndex, so the names read as members.  A DevBuf
// added here and left out of release_all() does not compile
struct FlatWork {
	DevBuf ws_q, ws_qn, ws_pd, ws_pi, ws_gthr, ws_add, ws_xi, ws_pbnd;
	DevBuf ws_flag, ws_tie;                        // inner-product boundary ties: flagged queries + tie-pass scratch
	DevBuf ws_pfq, ws_cand, ws_ex, ws_fail, ws_fb; // bf16x3 prefilter (csrc/flat_bf16.hip)
	DevBuf ws_e2, ws_stream, ws_sorttmp, ws_seg, ws_rowmask, ws_items1, ws_qcount; // coarse filter (csrc/flat_coarse.hip)
	DevBuf ws_fbk, ws_fbr, ws_seed;                // ... its bucketed finish
	DevBuf ws_cb16;                                // IVF coarse quantisation (csrc/coarse_bf16.hip)
	void release_all() { // the index leaves its device (FlatIndex::to_device)
		DevBuf *const all[] = {&ws_q,   &ws_qn,   &ws_pd,  &ws_pi,   &ws_gthr, &ws_add, &ws_xi,     &ws_pbnd,    &ws_flag, &ws_tie,     &ws_pfq,    &ws_cand,   &ws_ex,
		                       &ws_fail, &ws_fb,  &ws_e2,  &ws_stream, &ws_sorttmp, &ws_seg, &ws_rowmask, &ws_items1, &ws_qcount, &ws_fbk, &ws_fbr, &ws_seed, &ws_cb16};
		static_assert(sizeof all / sizeof *all * sizeof(DevBuf) == sizeof(FlatWork), "a workspace of FlatWork is missing from release_all()");
		for (DevBuf *b : all)
			b->release();
	}
};

class FlatIndex : public IndexBase, public FlatWork {
public:
	FlatGeom geom;
	float *vecs() const { // [cap][dp]
		return vecs_.get();
	}
	float *norms() const { // [cap]
		return norms_.get();
	}
	int64_t cap = 0;
	bool force_direct = false; // test hook: per-pair kernel for any nq
	bool force_staged = false; // test hook: LDS-staged flat_direct kernel instead of the packed scan kernel

	FlatIndex(int d, int metric);
	~FlatIndex() override;
	void reset();
	int64_t remove_ids(const mvs_search_params *sel, const int64_t *d_idmap = nullptr, RemoveMarks *marks = nullptr) override;
	void check_compatible_for_merge(IndexBase &other) override;
	void merge_from(IndexBase &other, int64_t add_id) override;
	void copy_rows_to_host(float *out); // logical [ntotal][d] rows (storage format undone)
	void recon_source(ReconSource &src, hipStream_t st) override;
	void add(int64_t n, const float *x) override;
	void add_device(int64_t n, const float *d_x, hipStream_t st) override;
	void search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I,
	                   const mvs_search_params *params, hipStream_t st) override;
	void search_mapped(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I,
	                   const mvs_search_params *params, const int64_t *d_idmap, hipStream_t st) override;
	void to_device(int new_device) override;
	IndexBase *clone(int on_device) override;
	void to_host(HostIndex &out) override;
	bool set_option(const char *key, int64_t v) override;
	// The search's host driver: the ENTRY (the only stage callers use), the TIE WRAPPER (inner product: the k + 1 request and its flags; a
	// re-run of unproven queries enters here), the ROUTE (which filter or exact kernel takes the pass)
	void search_flat(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I,
	                 const mvs_search_params *params, const int64_t *d_idmap, hipStream_t st);
	void tie_wrapped_search(const FlatSearchRequest &rq);
	void route(const FlatSearchRequest &r);
	void exact_pair_scan(const FlatSearchRequest &r);
	void exact_direct(const FlatSearchRequest &r);
	void exact_mfma(const FlatSearchRequest &r);
	void search_extra_metric(const FlatSearchRequest &r);
	// the exact branches' common tail: partial lists and threshold slots of `nparts` row ranges; their merge, the tie pass, kinfo
	void reserve_partials(const FlatSearchRequest &r, int64_t nparts);
	void finish_exact(const FlatSearchRequest &r, const ExactLaunch &x);
	// range search: the scan and its dispatch are csrc/range_search.hip's (range_search_mapped); the host entry and the statistic are csrc/index.hip's
	void range_search(int64_t nq, const float *x, float radius, const mvs_search_params *params, RangeResult &out) override;
	void range_search_mapped(int64_t nq, const float *d_x, float radius, const mvs_search_params *params, const int64_t *d_idmap,
	                         RangeResult &out, hipStream_t st) override;
	bool named_stat(const char *name, int64_t *v) override;
	RangeWork range_work;
	bool range_use_mfma = true; // option range_mfma = 0: BLAS-branch batches on the VALU kernel's formula mode (same bits)

	// The stores derived lazily from the rows before a search (csrc/dev_mem.h DevRowStore: capacity, rows converted so far and the padding
	// live in the store).  They and the blocks below free themselves; drop_bf16_rows / drop_i8 empty them when the rows change
	// bf16x3 prefilter (csrc/flat_bf16.hip): rows as bf16 hi/lo
	DevRowStore bf; // rows [bf.cap + 64][2 dp]: the kernel prefetches up to two tiles past the last row without clamping
	unsigned short *vecs_bf() const {
		return (unsigned short *)bf.rows.p;
	}
	DevBlock<unsigned> d_max_norm_bits; // [16] maxima over the rows as f32 bits: word 0 the largest squared row norm, the others the coarse store's (CL_NORM_* in csrc/flat_collect.h)
	int prefilter_mode = -1;            // option "prefilter": -1 auto, 0 off, 1 whenever the kernel supports the shape
	int64_t pf_last_fallback = 0;       // diagnostics: queries of the last search that were re-run
	int64_t pf_queries_total = 0, pf_fallback_total = 0;
	float pf_max_rel_err = 0.f; // largest observed |approx - exact| / (||x|| ||y||) among re-scored candidates
	// bf16 coarse filter (csrc/flat_collect.hip): rows as bf16 only, candidate stream, per-query bounds
	DevRowStore h1; // rows [h1.cap + 192][dp1] centred rows as bf16 (+ 192: unclamped prefetch of a 64-row block); side: beta
	unsigned short *vecs_h1() const {
		return (unsigned short *)h1.rows.p;
	}
	float *beta_h1() const { // [h1.cap + 192] -||y - mu||^2 (L2) or <mu, y> (inner product)
		return (float *)h1.side.p;
	}
	DevBlock<float> mu_h1; // [dp] the centre (mean of the rows present at the first build)
	// ---- what the coarse filter keeps BETWEEN searches (a pass itself travels in CollectRequest / CollectResult): option switches,
	// what earlier searches learnt about this index's data, statistics
	bool tie_from_candidates = true; // option tie_from_candidates = 0: inner-product ties re-scan the database (A/B, tests)
	bool cl_k32 = true;       // 16 < k <= 32 at d <= 128 on the coarse filter with 32 row classes (option cl_k32; 0: bf16x3 / f32 as before)
	bool cl_defer = true;     // option cl_defer_count
	// Round 5, bucketed finish of the d = 128 L2 coarse filter: final-bound filter -> the survivors into per-query row buckets -> one
	// wavefront per query re-scores them -> one wavefront per query selects and prints (csrc/ivf_collect.hip, shared with the IVF path):
	// no radix sort, no segments, ~ 4 x fewer rows re-scored.
	bool cl_fbucket = true;      // option cl_fbucket
	bool cl_bigk = true; // option cl_bigk: lists of 129 .. 2048 entries on the coarse filter (bounds from row ranges, frozen scan, segmented sort); 0: the exact kernels
	int cl_stream_cap_per_query = 0; // option cl_stream_cap (0: 4096 entries per query, at least 2^20)
	int64_t cl_cap_hint = 0;         // entries per query the last overflow asked for (the next search starts there)
	double cl_est_per_query = 0; // candidates per query of the last search: sizes the next search's sort (collect_sort_estimate)
	int cl_fpitch = 256;         // bucket entries per query (grows with the data: grow_bucket_pitch)
	bool cl_fbucket_off = false; // a query's bucket overflowed on this index's data: the sorted pipeline from then on
	int cl_skip = 0, cl_skip_len = 0; // searches that bypass the coarse filter after it gave up on this index's data (doubling, <= 64)
	int64_t cl_queries_total = 0, cl_candidates_total = 0, cl_overflows = 0, cl_last_candidates = 0, cl_heavy_total = 0;
	int64_t cl_scan_items = 0, cl_scan_ranges = 0; // the plan of the last d <= 128 scan launch (stats cl_scan_items / cl_scan_ranges)
	int64_t cl_last_rescored = -1, cl_rescored_total = 0, cl_rescored_queries = 0, cl_admitted_in_fb = 0; // bucketed finish: survivors of the final-bound filter
	void ensure_max_norm_bits(hipStream_t st);
	void ensure_bf16_rows(hipStream_t st);
	void ensure_h1_rows(hipStream_t st);
	// int8 coarse store (d <= 128, >= 262 144 rows; csrc/flat_collect.hip "int8 store"), next to the bf16 one: the scan, its pre-passes and the
	// big lists' pass A read it; the small-batch path and the IVF quantiser keep the bf16 store
	// rows [i8.cap + 256][128] clamp(rint(y' / sy)) (+ 256: the scan's unclamped prefetch of the 128-row stage behind the one that holds the
	// last row -- CL_SUB_I8 * CL_BN); side: beta
	DevRowStore i8;
	signed char *vecs_i8() const {
		return (signed char *)i8.rows.p;
	}
	int *beta_i8() const { // [i8.cap + 256] rint(beta / unit); INT_MIN: an outlier row
		return (int *)i8.side.p;
	}
	DevBlock<unsigned> d_i8_bits; // [4] max ||y' - sy Y||^2, max |beta / unit|, max |y'_i| (f32 bits)
	float i8_sy = 0.f, i8_unit = 0.f; // sy = 2^e, unit = alpha sy^2; the query scale is sa = alpha sy
	int i8_state = 0;  // 0: not decided yet, 1: the int8 store serves, -1: the bf16 store (until the store is rebuilt)
	bool cl_i8 = true; // option cl_i8 (0: the bf16 store)
	int cl_classes = 0;        // option cl_classes (tests: 16 | 32 row classes for k <= 16 on the int8 store; 0: collect_slot_stride's rule)
	int cl_row_classes = 0;    // class slots per query of the last coarse pass (stat cl_row_classes; 0: frozen bounds, no slots)
	bool ensure_i8_rows(hipStream_t st); // true: the int8 store is current and serves this search
	void drop_i8();
	DevBlock<int> d_outl; // [1 + CL_OUTL_CAP] outlier rows of the coarse-filter store: count, rows (csrc/flat_collect.hip "outlier rows")
	int h1_outliers = 0;   // ... their number as the host last read it (after a conversion)
	int64_t outl_total = 0; // (diagnostics: mvs_index_get_stat "flat_outlier_rows")
	bool outlier_rows = true; // option outlier_rows
	// IVF coarse quantisation: the np nearest rows (L2, FAISS order) by distance matrix + selection (csrc/coarse_select.hip);
	// false: shape not served, the caller uses search_device
	// need_matrix: the caller reads coarse_matrix() afterwards (the Flat shadow's proof); otherwise L2 quantisers of 16 < d <= 128 take the
	// bf16 filter + exact re-scoring of csrc/coarse_bf16.hip (round 6: no distance matrix at all, same output bit for bit)
	bool coarse_topk(int64_t nq, const float *d_x, int64_t np, float *d_D, int64_t *d_I, hipStream_t st, bool need_matrix = true);
	int64_t cb16_queries = 0; // queries served by csrc/coarse_bf16.hip (diagnostics)
	size_t cb16_stats_off = 0; // byte offset of the exhaustive-query counter in ws_cb16
	int64_t cb16_last_nq = 0;  // queries / offset of the per-query candidate counts of the last call (diagnostics)
	size_t cb16_ccount_off = 0;
	// what the last coarse_topk left behind (csrc/ivf.hip flat_shadow_search): the [nq][ntotal] distance matrix -- whole only when
	// the batch fitted one chunk --, and the rows' squared norms
	const float *coarse_matrix() const {
		return (const float *)ws_q.p;
	}
	bool coarse_matrix_covers(int64_t nq) const {
		return ntotal > 0 && nq <= std::max<int64_t>(64, ((int64_t)512 << 20) / (ntotal * 4) / 64 * 64);
	}
	const float *row_norms() const {
		return norms();
	}
	// One pass of the coarse filter and its stages (csrc/flat_coarse.hip).  CollectPlan is the shape of the pass, CollectWork what the
	// stages hand to one another (both defined there).
	CollectResult collect_candidates(const CollectRequest &rq);
	CollectPlan collect_plan(const CollectRequest &rq) const;
	void collect_workspaces(const CollectPlan &pl, int64_t nq, CollectWork &w);
	void collect_prepare(const CollectRequest &rq, const CollectPlan &pl, CollectWork &w);
	void collect_launch_scan(const CollectRequest &rq, const CollectPlan &pl, CollectWork &w);
	bool collect_scan(const CollectRequest &rq, const CollectPlan &pl, CollectWork &w, CollectResult &res);
	bool collect_relieve_overflow(const CollectRequest &rq, const CollectPlan &pl, CollectWork &w);
	bool collect_finish_bucketed(const CollectRequest &rq, const CollectPlan &pl, CollectWork &w, CollectResult &res);
	void collect_finish_sorted(const CollectRequest &rq, const CollectPlan &pl, CollectWork &w, CollectResult &res);
	bool grow_bucket_pitch(int64_t bmax, int64_t nq);
	void record_candidates(int64_t nq, int64_t ncand);
	bool deferred_count_overflowed(int64_t nq, int64_t deferred_cap);
	bool collect_settle(const CollectResult &cr, bool deferred, int64_t nq);
	void ensure_ctl_copy();
	PinnedMem cl_hdr_mem;
	CollectCtl *h_cl_hdr() const { // pinned copy of the control block's header (bucket statistics); null before ensure_ctl_copy()
		return (CollectCtl *)cl_hdr_mem.p;
	}
	// ---- shadow clustering (round 5): a Flat L2 index whose rows CLUSTER keeps an IVF index of the same rows and answers large
	// batches through it -- nprobe nearest lists by the coarse filter with per-list centring, then a proof per query that no other
	// list can matter; what cannot be proven is re-run on the Flat kernels.  Built lazily when the global-centring filter admits
	// thousands of candidates per query (clustered rows with large norms: 9 764 at the C3 mixture, 45.6 ms per batch).
	IndexBase *shadow = nullptr;
	int64_t shadow_rows = -1;  // ntotal the shadow holds
	int shadow_state = 0;      // 0 not wanted yet, 1 wanted / in use, -1 given up on this data (too many queries could not be proven)
	int shadow_mode = -1;      // option flat_shadow: -1 auto, 0 never, 1 from the first large search on
	int shadow_nprobe = 32;    // option flat_shadow_nprobe
	int64_t shadow_queries = 0, shadow_unproven = 0;
	int64_t shadow_trained_rows = 0; // ntotal when the clustering was trained (re-trained once the index has doubled)
	uint64_t mut_gen = 0, shadow_gen = 0; // generation of the rows (bumped by reset()) / the one the shadow was built from
	double shadow_build_seconds = 0;      // time spent building / extending the shadow (inside searches), mvs_index_shadow_stats
	int64_t shadow_builds = 0, shadow_extends = 0;
	bool shadow_sync(hipStream_t st);
	bool shadow_search(const FlatSearchRequest &rq); // false: the batch takes the normal path
	void drop_shadow();
	void set_timing(bool on) override {
		timing_enabled = on;
		if (shadow)
			shadow->set_timing(on);
	}
	void resolve_timing(int *count, double *total_ms) override { // (the dominant kernel of a shadow search is timed by the shadow index)
		resolve_kernel_timing(count, total_ms);
		if (shadow) {
			int c2 = 0;
			double t2 = 0;
			shadow->resolve_timing(&c2, &t2);
			if (count)
				*count += c2;
			if (total_ms)
				*total_ms += t2;
		}
	}
	void drop_bf16_rows();
	// the search through a filter (csrc/flat_coarse.hip).  false: not served, an exact kernel takes the pass (always so under
	// FlatSearchRequest::exact_only)
	bool search_prefilter(const FlatSearchRequest &r);
	bool search_prefilter_pass(const FlatSearchRequest &r, bool defer, bool *overflow);
	bool prefilter_route(const FlatSearchRequest &rq, PrefilterRoute &r) const;
	int prefilter_bf16x3(const FlatSearchRequest &r, int *fail_cnt, int *fail_q, CollectResult &cr);
	// the queries of `batch` a proof rejected, run again as a quiet request of their own (no re-entry through search_flat)
	void rerun_unproven(const FlatSearchRequest &batch, int nf, int *fail_q, bool exact_only);
	PinnedMem report_mem;
	CollectReport *h_report() const { // pinned: what a search tells the host (csrc/flat_collect.h); null before ensure_report()
		return (CollectReport *)report_mem.p;
	}
	void ensure_report();
	// row shard of a ShardedIndex (csrc/sharded.hip): results are the shard's ROW numbers in the pure order, no tie pass
	// (the sharded index resolves ties across shards); an id map passed to search_flat then only feeds the selector
	bool raw_rows = false;
	// tie pass for `nf` flagged queries: out[f][0..k) = the k smallest row ids with score >= d_T[f] (ascending, -1 padded)
	void tie_candidates(int64_t nf, const float *d_xf, const float *d_T, int64_t k, int64_t *d_rows_out, SelectorDev sel,
	                    const int64_t *d_selmap, hipStream_t st);
	void offset_rows(int64_t *d_rows, int64_t total, hipStream_t st); // += label_offset on valid entries
	// what the Flat scans test: d_idmap[row], or the row number
	IdDomain sel_domain(const int64_t *d_idmap) const {
		return IdDomain::rows(0, ntotal, d_idmap);
	}
	SelectorDev upload_selector(const mvs_search_params *p, const int64_t *d_selmap, hipStream_t st) {
		return selector.upload(p, sel_domain(d_selmap), st);
	}
	bool ip_exact_ties = true;   // option "ip_exact_ties" = 0: keep the pure (score desc, id asc) order (raw shard lists)
	void resolve_ip_ties(int64_t nq, const float *d_x, int64_t k, const TieFlags &fl, SelectorDev sel,
	                     const int64_t *d_idmap, float *d_D, int64_t *d_I, hipStream_t st, int64_t kraw = 0,
	                     const TieSource *ties = nullptr); // (ties == nullptr: the tied rows by a scan of the database, tie_candidates)
	SelectorHolder selector;
	hipStream_t last_search_stream = nullptr;
	bool have_last_search = false;
	void grow(int64_t need, hipStream_t st);
	// ---- ingest staging (round 6): DataChunk-sized adds are collected in a pinned slot and sent to the device once per slot ----
	PinnedRing add_ring;
	int pend_slot = -1, add_flip = 0;
	size_t pend_bytes = 0;
	int64_t pend_rows = 0, pend_row0 = 0; // rows of ntotal that are staged, not yet on the device / the first of them
	bool lazy_adds = true;                // option lazy_adds = 0: every add() goes to the device at once (round 5)
	int64_t add_flushes = 0;
	bool flush_adds();                    // true: rows were sent (on `stream`)
	struct Retired {
		DevBlock<float> vecs, norms;
		hipEvent_t done;
	};
	std::vector<Retired> retired; // row stores replaced by a growth: freed once the copy out of them has finished
	void reap_retired(bool wait);

private:
	DevBlock<float> vecs_, norms_;
	// a fresh pair for `rows` rows on the current device (both allocated, or it throws and nothing is held) ...
	void alloc_rows(int64_t rows, DevBlock<float> &nv, DevBlock<float> &nn) const;
	// ... takes the place of the index's pair, which is freed once what `st` holds so far has finished (reap_retired)
	void replace_rows(hipStream_t st, DevBlock<float> &&nv, DevBlock<float> &&nn);
};

class IDMapIndex : public IndexBase {
public:
	IndexBase *sub; // owned
	DevBlock<int64_t> ids; // [idcap]
	int64_t idcap = 0;
	PinnedRing id_ring; // (round 6) the ids of DataChunk-sized adds are staged like their rows
	int idp_slot = -1;
	size_t idp_bytes = 0;
	int64_t idp_row0 = 0;
	void flush_ids();

	explicit IDMapIndex(IndexBase *sub);
	~IDMapIndex() override;
	void adopt_tuning(const Tuning &t) override {
		tune_ = t;
		sub->adopt_tuning(t);
	}
	void refresh_trained() override {
		sub->refresh_trained();
		is_trained = sub->is_trained;
	}
	void train(int64_t n, const float *x) override;
	void add(int64_t n, const float *x) override;
	void add_with_ids(int64_t n, const float *x, const int64_t *ids) override;
	void add_device(int64_t n, const float *d_x, hipStream_t st) override;
	void add_with_ids_device(int64_t n, const float *d_x, const int64_t *d_ids, hipStream_t st) override;
	void search(int64_t nq, const float *x, int64_t k, float *D, int64_t *I, const mvs_search_params *params) override;
	void search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I,
	                   const mvs_search_params *params, hipStream_t st) override;
	void search_mapped(int64_t, const float *, int64_t, float *, int64_t *, const mvs_search_params *, const int64_t *,
	                   hipStream_t) override {
		throw_faiss("mvs::IDMapIndex::search_mapped", __FILE__, "nested IDMap is not supported");
	}
	void range_search(int64_t nq, const float *x, float radius, const mvs_search_params *params, RangeResult &out) override;
	void range_search_mapped(int64_t, const float *, float, const mvs_search_params *, const int64_t *, RangeResult &, hipStream_t) override {
		throw_faiss("mvs::IDMapIndex::range_search_mapped", __FILE__, "nested IDMap is not supported");
	}
	int64_t remove_ids(const mvs_search_params *sel, const int64_t *d_idmap = nullptr, RemoveMarks *marks = nullptr) override;
	bool is_idmap2 = false; // created as "IDMap2,..." (or read from an "IxM2" image): only check_compatible_for_merge tells the two apart
	void check_compatible_for_merge(IndexBase &other) override;
	void merge_from(IndexBase &other, int64_t add_id) override;
	void to_device(int new_device) override;
	IndexBase *clone(int on_device) override;
	void to_host(HostIndex &out) override;
	void set_label_offset(int64_t) override {
	}
	bool set_option(const char *key, int64_t v) override {
		return sub->set_option(key, v);
	}
	void set_timing(bool on) override {
		sub->set_timing(on);
	}
	void resolve_timing(int *count, double *total_ms) override {
		sub->resolve_timing(count, total_ms);
		kinfo = sub->kinfo;
	}

	void adopt_ids(const int64_t *xids, int64_t n); // image load: rows are already in `sub`
	void recon_source(ReconSource &src, hipStream_t st) override;
	ReconTable recon_tab; // external id -> row of the id map (dropped by add_with_ids, remove_ids, adopt_ids, to_device)

private:
	void grow_ids(int64_t need, hipStream_t st);
};

IndexBase *index_factory(int d, const char *description, int metric);
// rebuild a device index from its host image on the CURRENT default device (MVS_DEVICE / 0), or on `device` if >= 0
IndexBase *index_from_host(const HostIndex &h, int device = -1);
void stream_wait(hipStream_t waiter, hipStream_t signal);
void set_last_error(const char *what); // the calling thread's mvs_last_error text (csrc/index.hip)
void check_device(int dev); // throws FAISS's "Invalid GPU device" unless dev is one

// csrc/clustering.hip: faiss::Clustering on the device.  On return the assigner holds the k centroids learnt from the n rows
// of x (host, [n][assigner.d]); it works on the assigner's device and stream
struct KMeansSpec {
	int64_t k;
	int niter;
	bool spherical;
};
void kmeans_train(const KMeansSpec &s, int64_t n, const float *x, FlatIndex &assigner);

// csrc/ivf.hip
// The coarse side of an index with inverted lists (IVF<n>,Flat and the coded kinds): the quantiser that holds the nlist centroids, owned
struct CoarseSide {
	std::unique_ptr<IndexBase> quantizer; // FlatIndex, or an HNSW index ("IVF<n>_HNSW<M>,Flat"); null: no coarse side ("SQ8")
	int64_t nlist = 0;
	explicit operator bool() const {
		return (bool)quantizer;
	}
	FlatIndex *flat() const { // null for an HNSW quantiser
		return quantizer && quantizer->kind == MVS_KIND_FLAT ? static_cast<FlatIndex *>(quantizer.get()) : nullptr;
	}
	// the k nearest centroids of n device rows, on `st`: a Flat quantiser's distance matrix + selection (csrc/coarse_select.hip,
	// csrc/coarse_bf16.hip) where it serves the shape, else the quantiser's own search (hnsw_params: an HNSW quantiser's efSearch, or
	// null).  The quantiser's tuning is current afterwards: the owner calls its use_device()
	void topk(int64_t n, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *hnsw_params, hipStream_t st);
	void assign(int64_t n, const float *d_x, float *d_D, int64_t *d_I, hipStream_t st) { // k = 1: the list a row goes to
		topk(n, d_x, 1, d_D, d_I, nullptr, st);
	}
	void get_centroids(float *out);      // [nlist][d]
	void set_centroids(const float *c); // throws for an HNSW quantiser that already holds rows (a graph cannot be emptied)
	void adopt_tuning(const Tuning &t) {
		quantizer->adopt_tuning(t);
	}
	void to_host(HostIndex &out) { // the image's `sub`
		out.sub.reset(new HostIndex);
		quantizer->to_host(*out.sub);
	}
};
CoarseSide *coarse_side_of(IndexBase *ix); // null for "SQ8" and for a kind without inverted lists
IndexBase *make_ivf_index(int d, const std::string &desc, int metric); // nullptr if desc is not an IVF string
IndexBase *ivf_quantizer_of(IndexBase *ix);
int64_t ivf_nlist_of(IndexBase *ix);
bool ivf_get_centroids(IndexBase *ix, float *out);
bool ivf_set_centroids(IndexBase *ix, const float *c);
IndexBase *ivf_from_host(const HostIndex &h, int device);
// csrc/hnsw.hip
IndexBase *make_hnsw_index(int d, const std::string &desc, int metric);
bool hnsw_set_ef_construction(IndexBase *ix, int v);
int hnsw_get_ef_construction(IndexBase *ix); // -1 if not HNSW
int64_t hnsw_graph_info(IndexBase *ix, int *max_level, int *entry_point); // neighbour slots, -1 if not HNSW
bool hnsw_walk_stats(IndexBase *ix, double *evaluations, double *f32_rows, double *bf16_rows); // counters of the last timed search
bool hnsw_get_graph(IndexBase *ix, int32_t *levels, int64_t *offsets, int32_t *neighbors);
IndexBase *hnsw_from_host(const HostIndex &h, int device); // MVS_KIND_HNSW and MVS_KIND_HNSWSQ images
bool hnswsq_get_trained(IndexBase *ix, float *out); // "HNSW<M>,SQ8": what sq_get_trained / sq_set_trained / sq_get_codes do; false on another kind
bool hnswsq_set_trained(IndexBase *ix, const float *t);
bool hnswsq_get_codes(IndexBase *ix, int64_t row0, int64_t n, uint8_t *out);
// csrc/pq.hip
IndexBase *make_pq_index(int d, const std::string &desc, int metric); // nullptr if desc is not a PQ string
IndexBase *pq_from_host(const HostIndex &h, int device);
bool pq_info(const IndexBase *ix, int *M, int *nbits); // false if not a PQ index (as the three below)
bool pq_get_centroids(IndexBase *ix, float *out);
bool pq_set_centroids(IndexBase *ix, const float *c);
bool pq_get_codes(IndexBase *ix, int64_t row0, int64_t n, uint8_t *out);
// csrc/ivfpq.hip, csrc/sq.hip: the kinds over coded inverted lists.  Their coarse side and list view are CodedListsIndex's
// (csrc/coded_lists.h: coded_lists_of(ix) -> coarse, nlist, set_coarse, list_size, get_list)
IndexBase *make_ivfpq_index(int d, const std::string &desc, int metric); // nullptr if desc is not an "IVF<n>,PQ..." string
IndexBase *ivfpq_from_host(const HostIndex &h, int device);
bool ivfpq_info(const IndexBase *ix, int *M, int *nbits); // false if not an IVFPQ index (as the two below)
bool ivfpq_get_codebooks(IndexBase *ix, float *out);
bool ivfpq_set_codebooks(IndexBase *ix, const float *c);
IndexBase *make_sq_index(int d, const std::string &desc, int metric); // nullptr if desc is neither "SQ..." nor "IVF<n>,SQ..."
IndexBase *sq_from_host(const HostIndex &h, int device);             // MVS_KIND_SQ and MVS_KIND_IVFSQ images
bool sq_get_trained(IndexBase *ix, float *out);     // vmin [d] | vdiff [d]; false if neither SQ kind (as the next)
bool sq_set_trained(IndexBase *ix, const float *t);
bool sq_get_codes(IndexBase *ix, int64_t row0, int64_t n, uint8_t *out); // SQ8 only
// csrc/refine.hip
IndexBase *make_refine_index(int d, const std::string &desc, int metric, const std::string &full); // nullptr if desc does not end in ",RFlat" / ",Refine(...)"
IndexBase *refine_from_host(const HostIndex &h, int device);
IndexBase *refine_base_of(IndexBase *ix);  // nullptr / false if not a Refine index (as the ones below)
IndexBase *refine_store_of(IndexBase *ix);
bool refine_set_k_factor(IndexBase *ix, float k_factor);
bool refine_get_k_factor(IndexBase *ix, float *k_factor);
// csrc/pretransform.hip
IndexBase *make_pretransform_index(int d, const std::string &desc, int metric, const std::string &full,
                                   IndexBase *(*sub_factory)(int, const std::string &, int, const std::string &)); // nullptr if desc does not begin with a vector transform
IndexBase *pretransform_from_host(const HostIndex &h, int device);
IndexBase *pretransform_sub_of(IndexBase *ix); // nullptr / -1 if not a PreTransform index (as the two below); the others throw
int pretransform_count(IndexBase *ix);
int pretransform_out_dim(IndexBase *ix);
void pretransform_info(IndexBase *ix, int i, int *type, int *d_in, int *d_out, int *have_bias, int *is_trained);
void pretransform_get_linear(IndexBase *ix, int i, float *A, float *b);
void pretransform_set_linear(IndexBase *ix, int i, const float *A, const float *b);
void pretransform_get_pca(IndexBase *ix, int i, float *mean, float *eigenvalues);
void pretransform_apply(IndexBase *ix, int64_t n, const float *x, float *out);
void pretransform_apply_device(IndexBase *ix, int64_t n, const float *d_x, float *d_out, hipStream_t st);
// csrc/io.cpp-ish (index_io.hip)
void write_index_file(IndexBase *ix, const char *filename);
IndexBase *read_index_file(const char *filename);
// csrc/sharded.hip: one index over several devices behind the same surface
std::vector<int> shard_devices_from_env(); // env MVS_DEVICES="0,1,...,7" (empty / unset: no sharding)
IndexBase *make_sharded_index(int d, const char *desc, int metric, const std::vector<int> &devices);
IndexBase *shard_from_host(const HostIndex &h, const std::vector<int> &devices);
bool is_sharded(const IndexBase *ix);
IndexBase *sharded_inner_view(IndexBase *ix); // the index the glue's dynamic_casts should see (ix itself if unsharded)
void sharded_for_each(IndexBase *ix, const std::function<void(IndexBase *)> &f);
int sharded_info(const IndexBase *ix, int *devices, int max_devices, int64_t *rows_per_shard, int64_t *last_flagged);
// csrc/merge_host.hip
void merge_shards_raw_host(int metric, int64_t n, int64_t kk, int nshard, const float *D, const int64_t *I, float *D_out,
                           int64_t *I_out);
void finish_ip_ties_host(int64_t n, int64_t k, int64_t kk, const float *raw_v, const int64_t *raw_g, int64_t nf,
                         const int64_t *fq, const int64_t *first, float *D_out, int64_t *I_out);
void merge_shards_host(int metric, int64_t n, int64_t k, int nshard, const float *D, const int64_t *I, float *D_out,
                       int64_t *I_out);

} // namespace mvs

struct mvs_range_result { // faiss::RangeSearchResult's arrays, in host memory (filled by csrc/index.hip and csrc/binary.hip)
	mvs::RangeResult res;
};
