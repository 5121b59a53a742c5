// csrc/ivfpq_tables.h -- launchers of the two table kernels behind "IVF<n>,PQ<M>"'s option ivfpq_precomputed_table
// (csrc/ivfpq_tables.hip; the contract is include/mi355_faiss.h "precomputed tables").
#pragma once
#include "common.h"

#include <cstdint>

namespace mvs {

constexpr int IVFPQ_QT_QUERIES = 64; // queries one workgroup of ivfpq_query_table_kernel takes

// L [nlist][M][256] = fmaf(2, <c_m, p>, <p, p>) from the centroids [nlist][d] and the codebooks [M][256][dsub], on `st`
void launch_ivfpq_list_table(const float *d_cent, const float *d_cb, int64_t nlist, int d, int M, float *d_L, hipStream_t st);
// S [nqc][M][256] = <x_m, p> of the queries [nqc][d], on the f32 matrix pipe, on `st`
void launch_ivfpq_query_table(const float *d_xq, int64_t nqc, int d, int M, const float *d_cb, float *d_S, hipStream_t st);

} // namespace mvs
