// compat/faiss/IndexPreTransform.h -- faiss::IndexPreTransform over the device's "<t1>,...,<tn>,<sub>" index (MVS_KIND_PRETRANSFORM).  It is
// no IndexIVF: the glue's dynamic_cast<faiss::IndexIVF *> (src/faiss_extension.cpp:675) fails on it as it does on FAISS's own class, so SQL
// sets no nprobe on a "PCA64,IVF4096,Flat" (the sub-index's own nprobe, default 1, applies); `index` is the sub-index for a host that
// unwraps it itself.
#pragma once
#include "Index.h"
#include "VectorTransform.h"
#include <vector>
namespace faiss {
struct IndexPreTransform : Index {
	std::vector<VectorTransform *> chain; // views of the device chain's slots (owned by this wrapper)
	Index *index = nullptr;               // a borrowed view of the sub-index (owned by the device object)
	bool own_fields = false;
	~IndexPreTransform() override;
	void refresh_chain() override;
	void before_add() override;
	void before_search() const override;
	// IndexPreTransform::apply_chain: n rows of d floats -> a new[] array of n rows of the chain's output dimension (the caller delete[]s it)
	const float *apply_chain(idx_t n, const float *x) const;
};
} // namespace faiss
