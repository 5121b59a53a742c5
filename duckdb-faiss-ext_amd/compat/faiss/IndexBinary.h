// compat/faiss/IndexBinary.h -- faiss::IndexBinary over the C ABI's mvs_binary_index (include/mi355_faiss.h "binary indexes"): vectors
// of d bits as code_size = d / 8 bytes, Hamming distances as int32.  Written against FAISS's public interface (member and method names
// as FAISS documents them); d / code_size / ntotal are refreshed after every mutating call.
#pragma once
#include "Index.h"

#include <cstdint>
namespace faiss {

struct IndexBinary {
	using distance_t = int32_t;
	int d = 0;         // bits
	int code_size = 0; // bytes per vector
	idx_t ntotal = 0;
	bool verbose = false;
	bool is_trained = true;
	MetricType metric_type = METRIC_L2;

	virtual ~IndexBinary();
	virtual void train(idx_t n, const uint8_t *x); // a no-op
	virtual void add(idx_t n, const uint8_t *x);
	virtual void add_with_ids(idx_t n, const uint8_t *x, const idx_t *xids);
	// the k smallest (distance, internal row) pairs per query; missing slots are distance 2147483647 with label -1
	virtual void search(idx_t n, const uint8_t *x, idx_t k, int32_t *distances, idx_t *labels, const SearchParameters *params = nullptr) const;
	// every row with ham < radius, strict, in row order; distances as float, as FAISS's RangeSearchResult stores them
	virtual void range_search(idx_t n, const uint8_t *x, int radius, RangeSearchResult *result, const SearchParameters *params = nullptr) const;
	virtual void reset();
	virtual void reconstruct(idx_t key, uint8_t *recons) const;
	virtual void reconstruct_n(idx_t i0, idx_t ni, uint8_t *recons) const;
	// FAISS's base-class refusal: removal is out of scope for the binary family
	virtual size_t remove_ids(const IDSelector &sel);
	// ... and so is merging: "merge_from() not implemented" / "check_compatible_for_merge() not implemented"; both indexes stay untouched
	virtual void merge_from(IndexBinary &otherIndex, idx_t add_id = 0);
	virtual void check_compatible_for_merge(const IndexBinary &otherIndex) const;

	// --- adaptor plumbing (not part of FAISS) ---
	mvs_binary_index *handle = nullptr;
	bool owns_handle = true;
	virtual void refresh();
	static IndexBinary *wrap(mvs_binary_index *h, bool owned); // an IndexBinaryFlat, or an IndexBinaryIDMap around one
};

} // namespace faiss
