#pragma once
#include "../MetricType.h"
#include "StandardGpuResources.h"

#include <cstdint>
namespace faiss {
namespace gpu {
// faiss/gpu/GpuDistance.h: brute-force k-NN on matrices the caller owns, on the device (include/mi355_faiss.h "brute-force k-NN on
// caller-owned matrices").  Field names and defaults are FAISS's.  All pointers are device pointers on `device`; F32, F16 and BF16 are
// served for either matrix, metricArg and use_cuvs are accepted and ignored
enum class DistanceDataType { F32 = 1, F16, BF16 };
enum class IndicesDataType { I64 = 1, I32 };
struct GpuDistanceParams {
	faiss::MetricType metric = METRIC_L2;
	float metricArg = 0;
	int k = 0; // -1: all pairwise distances into outDistances [numQueries][numVectors]
	int dims = 0;
	const void *vectors = nullptr;
	DistanceDataType vectorType = DistanceDataType::F32;
	bool vectorsRowMajor = true;
	int64_t numVectors = 0; // (FAISS: idx_t)
	const float *vectorNorms = nullptr;
	const void *queries = nullptr;
	DistanceDataType queryType = DistanceDataType::F32;
	bool queriesRowMajor = true;
	int64_t numQueries = 0;
	float *outDistances = nullptr;
	bool ignoreOutDistances = false;
	IndicesDataType outIndicesType = IndicesDataType::I64;
	void *outIndices = nullptr;
	int device = -1; // -1: the current device
	bool use_cuvs = false;
};
void bfKnn(GpuResourcesProvider *resources, const GpuDistanceParams &args);
} // namespace gpu
} // namespace faiss
