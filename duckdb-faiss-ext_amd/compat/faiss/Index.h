// compat/faiss/Index.h -- faiss::Index as the reference's glue sees it, implemented over the C ABI of
// libmi355faiss.so (include/mi355_faiss.h).  Data members d / ntotal / is_trained are read directly by the glue
// (src/faiss_extension.cpp:159,355,490,518) and are refreshed after every mutating call.
#pragma once
#include "MetricType.h"
#include "impl/AuxIndexStructures.h"
#include "impl/FaissException.h"
#include "impl/IDSelector.h"

#include "../../../include/mi355_faiss.h"

#include <cstddef>
namespace faiss {

struct SearchParameters {
	IDSelector *sel = nullptr; // src/faiss_extension.cpp:678,694,719
	virtual ~SearchParameters() {
	}
};

struct Index {
	int d = 0;
	idx_t ntotal = 0;
	bool verbose = false;
	bool is_trained = true;
	MetricType metric_type = METRIC_L2;
	float metric_arg = 0;

	virtual ~Index();
	virtual void train(idx_t n, const float *x);                              // :396,:583
	virtual void add(idx_t n, const float *x);                                // :512,:609
	virtual void add_with_ids(idx_t n, const float *x, const idx_t *xids);    // :510,:607
	virtual void search(idx_t n, const float *x, idx_t k, float *distances, idx_t *labels,
	                    const SearchParameters *params = nullptr) const;      // :631
	// every row with dis < radius (L2) / dis > radius (inner product), strict; fills result->lims, allocates and fills labels and
	// distances.  Kinds that do not serve it throw "range search not implemented" (include/mi355_faiss.h "range search")
	virtual void range_search(idx_t n, const float *x, float radius, RangeSearchResult *result,
	                          const SearchParameters *params = nullptr) const;

	// the rows whose id is a member of sel go; returns their number.  IDSelectorBitmap and IDSelectorBatch only; kinds that do not serve it
	// throw "remove_ids not implemented for this type of index" (include/mi355_faiss.h "remove_ids").  ntotal is refreshed on this
	// wrapper and on every wrapper in its chain
	virtual size_t remove_ids(const IDSelector &sel);

	// otherIndex's rows follow this index's on the device and otherIndex ends empty (an IVF kind: stored id + add_id; Flat-codes kinds take
	// add_id = 0 only).  Kinds that do not serve it throw "merge_from() not implemented" / "check_compatible_for_merge() not implemented"
	// (include/mi355_faiss.h "merge_from and copy_subset_to").  ntotal is refreshed on both wrappers and their chains
	virtual void merge_from(Index &otherIndex, idx_t add_id = 0);
	virtual void check_compatible_for_merge(const Index &otherIndex) const;

	// the row as the index stores it, as d floats (include/mi355_faiss.h "reconstruct"): by key, by a range of keys, by a batch of keys, and
	// together with a search (a label of -1: every byte of the row 0xFF).  Kinds that do not serve it throw "reconstruct not implemented
	// for this type of index"
	virtual void reconstruct(idx_t key, float *recons) const;
	virtual void reconstruct_batch(idx_t n, const idx_t *keys, float *recons) const;
	virtual void reconstruct_n(idx_t i0, idx_t ni, float *recons) const;
	virtual void search_and_reconstruct(idx_t n, const float *x, idx_t k, float *distances, idx_t *labels, float *recons,
	                                    const SearchParameters *params = nullptr) const;

	// --- adaptor plumbing (not part of FAISS) ---
	mvs_index *handle = nullptr;
	bool owns_handle = true;
	void refresh();
	virtual void refresh_chain() { // refresh() here and on the wrappers of the sub-indexes
		refresh();
	}
	static Index *wrap(mvs_index *h, bool owned); // builds the IndexIDMap / IndexIVF / IndexHNSW / IndexFlat graph
	// pushes members the glue assigns directly on the wrapper (IndexHNSW::hnsw.efConstruction, :136-139) to the
	// device index before rows arrive; wrappers forward it down the chain
	virtual void before_add() {
	}
	// the same for members read at search time (IndexRefine::k_factor)
	virtual void before_search() const {
	}
};

[[noreturn]] void throw_last_error();
void fill_params(const Index *index, const SearchParameters *params, mvs_search_params *out);

} // namespace faiss
