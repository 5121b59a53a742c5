// csrc/coded_lists.h -- the host driver under the index kinds whose rows are CODES in inverted lists: "IVF<n>,PQ<M>" (csrc/ivfpq.hip),
// "IVF<n>,SQ8" and "SQ8" (csrc/sq.hip; SQ8 is the one-list case without a quantiser).  csrc/coded_lists.hip holds the code.  A kind
// derives from CodedListsIndex and supplies its parameters (codebooks / range), its encoder and its scan kernel; everything around the
// scan -- coarse side, code store, list view, units, selection, images, placement -- is here once.
#pragma once
#include "index.h"
#include "list_directory.h"

namespace mvs {

// rows of `pitch` code bytes on the device, in arrival order (also the whole store of csrc/pq.hip's "PQ<M>")
struct CodeStore {
	DevMem mem;
	unsigned char *codes() const { // [cap][pitch]
		return (unsigned char *)mem.p;
	}
	int64_t cap = 0;
	const int pitch; // code bytes per row, a multiple of 16
	explicit CodeStore(int code_size) : pitch((code_size + 15) / 16 * 16) {
	}
	void grow(int64_t need, int64_t ntotal, hipStream_t stream); // zero-filled beyond the `ntotal` rows it keeps
	void release() {
		mem.release();
		cap = 0;
	}
	// remove_ids (csrc/remove_ids.hip): a fresh zero-filled allocation of `cap` rows receives the survivors of `m` in their order /
	// rows perm[0 .. n) of the old one; the old allocation is freed.  If anything fails the store is as before
	void compact(const RemoveMarks &m, hipStream_t stream);
	void gather(const std::vector<int32_t> &perm, hipStream_t stream);
};

// what every scan kernel of a coded-lists kind is launched with (csrc/sq.hip's kernel takes it as it is, csrc/ivfpq.hip's extends it)
struct CodedScan {
	const unsigned char *codes; // rows of `pitch` bytes: list-sorted, or (no quantiser) the arrival-order store
	const long long *lids;      // their stored ids; null (no quantiser): the row number
	const long long *list_off;  // [nlist + 1]
	const float *cent;          // [nlist][d]; null (no quantiser): no centroid
	const float *par;           // the kind's parameters: codebooks [M][256][dsub] | range [4][d] vmin | vdiff | a | s
	const float *xq;            // the chunk's queries [nqc][d]
	const unsigned *pref;       // the chunk's ordinal bases [nqc][np + 1]
	const int2 *pairs;          // the unit's (query, rank) pairs grouped by list
	const int *poff, *goff;     // [nlist + 1]
	const unsigned *thr;        // [nqc] bounds
	unsigned long long *bucket; // [nqc][R]
	unsigned *cnt;              // [nqc]
	int *overflow;
	const long long *idmap;
	long long id0; // no quantiser: label of row 0 without an id map
	int nlist, d, pitch, np;
	long long p0, p1; // the unit's position window
	SelectorDev sel;
};

// Every device workspace and derived view a CodedListsIndex keeps between calls, and nothing else: a base of it, so the names read as
// members.  A DevBuf added here and left out of release_all() does not compile (as FlatWork, csrc/index.h)
struct CodedWork {
	DevBuf ws_add, ws_lab, ws_kind; // staged rows, their labels, scratch of the kind's own (residuals | partial ranges)
	DevBuf lcodes, lids, list_off_dev, cent_dev;
	DevBuf ws_cD, ws_cI, ws_pref, ws_pairs, ws_grp, ws_bucket, ws_list, ws_ctl;
	void release_all() { // the index leaves its device (CodedListsIndex::to_device)
		DevBuf *const all[] = {&ws_add, &ws_lab, &ws_kind, &lcodes,   &lids,   &list_off_dev, &cent_dev, &ws_cD,
		                       &ws_cI,  &ws_pref, &ws_pairs, &ws_grp, &ws_bucket, &ws_list,      &ws_ctl};
		static_assert(sizeof all / sizeof *all * sizeof(DevBuf) == sizeof(CodedWork), "a workspace of CodedWork is missing from release_all()");
		for (DevBuf *b : all)
			b->release();
	}
};

class CodedListsIndex : public IndexBase, protected CodedWork {
public:
	struct Names {                            // what the kind is called in error texts and statistics
		const char *cls, *file;               // "mvs::IVFPQIndex", its source file
		const char *label, *image;            // "IVFPQ" | "SQ8" in search's refusal of a large k; "IVFPQ" | "IVFSQ" in an image's
		const char *add_fn, *add_file;        // the FAISS function / file whose 'is_trained' check add fails
		const char *stat;                     // prefix of the named statistics: "ivfpq" | "sq"
		std::vector<uint8_t> HostIndex::*flat; // no quantiser: the image's field of codes [ntotal][code_size]
	};
	const Names names;
	CoarseSide coarse; // a Flat quantiser of nlist centroids; empty: one list that is the arrival-order store (SQ8)
	const int64_t nlist;
	const int code_size; // bytes of a row's code (M | d)
	int64_t nprobe = 1;
	bool have_par = false; // the kind's parameters are present: trained once the quantiser (if any) holds its centroids too
	float *d_par() const { // [par_floats]; null until ensure_par()
		return par_.get();
	}
	const size_t par_floats;
	CodeStore store;
	ListDirectory dir; // list and stored id of every row of the store (with a quantiser only)
	// the list view, rebuilt lazily
	bool dirty = true, cent_dirty = true;
	std::vector<int64_t> list_off, sid_h, top_rows; // top_rows[i]: rows of the i largest lists together
	int64_t nsorted = 0, max_list = 0;
	int64_t last_launches = 0, last_rescans = 0;

	CodedListsIndex(int kind, int d, int metric, int64_t nlist /* 0: no quantiser */, int code_size, size_t par_floats, bool window_one_rank,
	                const Names &names);
	~CodedListsIndex() override;
	void adopt_tuning(const Tuning &t) override;
	void set_coarse(const float *c); // coarse.set_centroids under this kind's trained-state rules
	// list view
	int64_t list_size(int64_t l);
	void get_list(int64_t l, int64_t *ids, uint8_t *codes); // ids [size], codes [size][code_size]; either may be null
	// add, search
	void set_label_offset(int64_t off) override;
	void add(int64_t n, const float *x) override;
	void add_with_ids(int64_t n, const float *x, const int64_t *ids) override;
	void add_device(int64_t n, const float *d_x, hipStream_t st) override;
	void add_with_ids_device(int64_t n, const float *d_x, const int64_t *d_ids, hipStream_t st) override;
	void search_mapped(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, const int64_t *d_idmap,
	                   hipStream_t st) override;
	void search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, hipStream_t st) override;
	int64_t remove_ids(const mvs_search_params *sel, const int64_t *d_idmap = nullptr, RemoveMarks *marks = nullptr) override;
	// csrc/merge.hip: code size, coarse centroids and parameters (codebooks / range) must agree bit for bit; the code rows travel as bytes
	void check_compatible_for_merge(IndexBase &other) override;
	void merge_from(IndexBase &other, int64_t add_id) override;
	void copy_subset_to(IndexBase &other, int subset_type, int64_t a1, int64_t a2) override;
	void recon_source(ReconSource &src, hipStream_t st) override;
	ReconTable recon_tab; // stored id -> arrival position, with the rows' lists (a quantiser only; dropped wherever `dirty` is set)
	bool named_stat(const char *name, int64_t *value) override; // <stat>_pair_block | _rows_per_workgroup | _scan_launches | _scan_rescans
	size_t device_bytes() const override;
	// images, placement
	void to_host(HostIndex &out) override;
	void load_image(const HostIndex &h); // an empty index on its device <- parameters and rows of the image (the quantiser is loaded by the caller)
	void to_device(int new_device) override;
	IndexBase *clone(int on_device) override;

protected:
	void update_trained();
	void ensure_par();
	const float *centroids_dev(); // [nlist][d] row-major copy of the quantiser's rows (on `stream`); null without a quantiser
	void assign_device(int64_t n, const float *d_x, float *d_D, int64_t *d_I); // the quantiser's k = 1 label of n device rows (on `stream`)
	void train_coarse(int64_t n, const float *x); // kmeans_train: the centroids IVF<nlist>,Flat of the same metric learns; the parameters are forgotten
	// ---- what the kind supplies
	virtual void check_empty_for_training() const = 0;        // throws once rows are encoded with the centroids / parameters
	virtual void check_image(const HostIndex &h) const = 0;  // the image's parameters and list (or code) counts fit this index
	virtual void params_to_host(HostIndex &out) = 0;
	virtual void params_from_host(const HostIndex &h) = 0;   // (sets them only where the image has them)
	// codes of rows [first_row, first_row + nb) from d_x and, with a quantiser, their lists d_lab (on `stream`)
	virtual void encode_block(int64_t nb, const float *d_x, const int64_t *d_lab, int64_t first_row) = 0;
	virtual int pair_block() const = 0; // Q: (query, rank) pairs of one list a scan workgroup takes
	// the scan kernel for one unit over `grid` = (pair groups, segments of R positions), and kinfo; rows: what a query can meet in the unit
	virtual void launch_scan_kernel(const CodedScan &a, dim3 grid, int64_t nqc, double rows) = 0;

private:
	struct Chunk { // one chunk of queries: device state of its selection, the scan's fixed arguments
		int64_t nqc;
		int k, Q, np;
		const int64_t *cI;
		unsigned long long *list;
		int *len, *gcnt, *gcur, *poff, *goff;
		CodedScan a;
	};
	const bool window_one_rank; // a unit of one rank is walked in windows [0, R), [R, 3R), [3R, 9R), ... (csrc/pq.hip's ranges)
	DevBlock<float> par_;
	PinnedMem h_flag; // one int: a scan's overflow flag
	SelectorHolder selector;
	void free_device();
	void check_trained_for_add() const;
	void check_rows(int64_t n) const; // the 2^31 guard
	void add_core_device(int64_t n, const float *d_x, const int64_t *ids_host);
	void add_host(int64_t n, const float *x, const int64_t *ids);
	void build_lists();
	void lists_changed(); // rows left or arrived behind add()'s back (remove_ids, merge_from, copy_subset_to): the view and the lookup table are derived again
	const unsigned char *list_codes() const;
	int64_t unit_rows(int ra, int rb, int64_t p0, int64_t p1) const;
	void launch_scan(Chunk &c, int ra, int rb, int64_t p0, int64_t p1);
	void scan_unit(Chunk &c, int ra, int rb, int64_t p0, int64_t p1);
};

CodedListsIndex *coded_lists_of(IndexBase *ix); // null if ix is not of a coded-lists kind

} // namespace mvs
