#pragma once
#include "../Index.h"
#include "StandardGpuResources.h"
namespace faiss {
namespace gpu {
// src/gpu/gpu.cpp:48.  Indexes are device-native already; this returns a new index object that lives on `device`
// (the glue replaces entry.index with it and drops the old one).
faiss::Index *index_cpu_to_gpu(GpuResourcesProvider *provider, int device, const faiss::Index *index);
// faiss/gpu/GpuClonerOptions.h.  useFloat16 turns a Flat or IDMap,Flat source into a half-precision Flat index (include/mi355_faiss.h
// "half-precision Flat"); the other members are accepted and ignored
enum IndicesOptions { INDICES_CPU = 0, INDICES_IVF = 1, INDICES_32_BIT = 2, INDICES_64_BIT = 3 };
struct GpuClonerOptions {
	IndicesOptions indicesOptions = INDICES_64_BIT;
	bool useFloat16CoarseQuantizer = false;
	bool useFloat16 = false;
	bool usePrecomputed = false;
	long reserveVecs = 0;
	bool storeTransposed = false;
	bool verbose = false;
	bool use_cuvs = false;
	bool allowCpuCoarseQuantizer = false;
};
faiss::Index *index_cpu_to_gpu(GpuResourcesProvider *provider, int device, const faiss::Index *index, const GpuClonerOptions *options);
} // namespace gpu
} // namespace faiss
