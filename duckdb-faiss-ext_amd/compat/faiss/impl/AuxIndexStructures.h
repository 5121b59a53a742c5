// compat/faiss/impl/AuxIndexStructures.h -- faiss::RangeSearchResult, the variable-length result of Index::range_search: query q's
// hits are entries [lims[q], lims[q + 1]) of labels and distances.  Written against FAISS's public interface (member names, constructor
// and do_allocation as FAISS documents them); the arrays are new[]-allocated and owned by the object.
#pragma once
#include "../MetricType.h"

#include <cstddef>
namespace faiss {

struct RangeSearchResult {
	size_t nq;    // number of queries
	size_t *lims; // size nq + 1
	idx_t *labels = nullptr;    // size lims[nq]
	float *distances = nullptr; // size lims[nq]
	size_t buffer_size;         // size of the result buffers FAISS's partial results use (kept for source compatibility)

	// lims is allocated (and zeroed) unless alloc_lims is false
	explicit RangeSearchResult(size_t nq, bool alloc_lims = true) : nq(nq), lims(nullptr), buffer_size(1024 * 256) {
		if (alloc_lims)
			lims = new size_t[nq + 1]();
	}
	// called once lims[nq] is known: allocates labels and distances
	virtual void do_allocation() {
		delete[] labels;
		delete[] distances;
		const size_t n = lims[nq];
		labels = new idx_t[n];
		distances = new float[n];
	}
	virtual ~RangeSearchResult() {
		delete[] labels;
		delete[] distances;
		delete[] lims;
	}
	RangeSearchResult(const RangeSearchResult &) = delete;
	RangeSearchResult &operator=(const RangeSearchResult &) = delete;
};

} // namespace faiss
