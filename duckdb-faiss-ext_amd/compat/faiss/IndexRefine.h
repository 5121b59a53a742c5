// compat/faiss/IndexRefine.h -- faiss::IndexRefine / faiss::IndexRefineFlat over the device's "<base>,RFlat" index (MVS_KIND_REFINE).  Neither
// is an IndexIVF: the glue's dynamic_cast<faiss::IndexIVF *> (src/faiss_extension.cpp:675) fails on it as it does on FAISS's own class, so
// SQL sets no nprobe on an "IVF...,RFlat" (the base's own nprobe, default 1, applies).
#pragma once
#include "Index.h"
namespace faiss {
struct IndexRefine : Index {
	Index *base_index = nullptr;   // borrowed views of the two sub-indexes (owned by the device object)
	Index *refine_index = nullptr;
	bool own_fields = false, own_refine_index = false;
	float k_factor = 1; // read at every search: an assignment on the wrapper reaches the device index
	~IndexRefine() override;
	void before_search() const override;
};
struct IndexRefineFlat : IndexRefine {};
} // namespace faiss
