// compat/faiss/IndexIVF.h -- IndexIVF::quantizer (src/faiss_extension.cpp:680), SearchParametersIVF (:677-686)
#pragma once
#include "Index.h"
#include "invlists/InvertedLists.h"
namespace faiss {
struct SearchParametersIVF : SearchParameters {
	size_t nprobe = 1;
	size_t max_codes = 0;
	SearchParameters *quantizer_params = nullptr;
};
struct IndexIVF : Index {
	Index *quantizer = nullptr; // borrowed view
	size_t nlist = 0;
	size_t nprobe = 1;
	// the entries a subset type selects are appended to other's lists, ids unchanged; this index is unchanged (the bare IVF kinds;
	// include/mi355_faiss.h "merge_from and copy_subset_to").  other's ntotal is refreshed
	virtual void copy_subset_to(IndexIVF &other, InvertedLists::subset_type_t subset_type, idx_t a1, idx_t a2) const;
	~IndexIVF() override;
};
struct IndexIVFFlat : IndexIVF {};
// faiss::IndexIVFPQ over the device's IVF<n>,PQ<M> index (MVS_KIND_IVFPQ): an IndexIVF -- the glue's cast at :675 reaches it --, not an IndexPQ
struct ProductQuantizer {
	size_t d = 0, M = 0, nbits = 8, dsub = 0, ksub = 256, code_size = 0;
};
struct IndexIVFPQ : IndexIVF {
	ProductQuantizer pq;
	bool by_residual = true;
};
// faiss::IndexScalarQuantizer / faiss::IndexIVFScalarQuantizer over the device's SQ8 / IVF<n>,SQ8 indexes (MVS_KIND_SQ / MVS_KIND_IVFSQ): the
// first is a plain Index -- none of the glue's casts reaches it --, the second an IndexIVF (:675 sets nprobe on it)
struct ScalarQuantizer {
	enum QuantizerType { QT_8bit = 0 };
	QuantizerType qtype = QT_8bit;
	size_t d = 0, bits = 8, code_size = 0;
};
struct IndexScalarQuantizer : Index {
	ScalarQuantizer sq;
};
struct IndexIVFScalarQuantizer : IndexIVF {
	ScalarQuantizer sq;
	bool by_residual = true;
};
} // namespace faiss
