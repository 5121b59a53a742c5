// csrc/pqfs_kernels.h -- what the two kinds with 4-bit fast-scan codes share (csrc/pqfs.hip "PQ<M>x4fs", csrc/ivfpqfs.hip
// faiss::IndexIVFPQFastScan): the chain of a table entry, the 8-bit quantisation of one sub-quantiser's 16 entries and the one-hot
// expansion of a code into the int8 MFMA's B operand.  Internal linkage, as csrc/pq_kernels.h.
#pragma once
#include "index.h"

#include <cfloat>

namespace mvs {

namespace {

constexpr int PQFS_KSUB = 16;
constexpr int PQFS_MAX_M = 128;

typedef int pqfs_i32x4 __attribute__((ext_vector_type(4)));

// the chain between query / row sub-vector xv and centroid c
__device__ __forceinline__ float pqfs_chain(const float *__restrict__ xv, const float *__restrict__ c, int dsub, int is_l2) {
	float acc = 0.f;
	if (is_l2) {
		for (int k = 0; k < dsub; ++k) {
			const float t = xv[k] - c[k];
			acc = fmaf(t, t, acc);
		}
	} else {
		for (int k = 0; k < dsub; ++k)
			acc = fmaf(xv[k], c[k], acc);
	}
	return acc;
}

// the 16 table entries Tm of one sub-quantiser -> the A operand's 16 bytes tq - 128 (the MFMA's operands are signed),
// tq = clamp((int)floorf(fmaf(T - lo, a, 0.5f)), 0, 255)
__device__ __forceinline__ pqfs_i32x4 pqfs_quantise16(const float *__restrict__ Tm, float lo, float a) {
	unsigned w[4] = {0, 0, 0, 0};
	for (int j = 0; j < PQFS_KSUB; ++j) {
		int v = (int)floorf(fmaf(__fsub_rn(Tm[j], lo), a, 0.5f));
		v = v < 0 ? 0 : (v > 255 ? 255 : v);
		w[j >> 2] |= (unsigned)((v - 128) & 255) << ((j & 3) * 8);
	}
	return pqfs_i32x4 {(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
}

// the 16-byte one-hot operand of a code: a single 1 at byte `code`
__device__ __forceinline__ pqfs_i32x4 pqfs_one_hot(unsigned code) {
	const unsigned v = 1u << ((code & 3u) * 8u), w = code >> 2;
	return pqfs_i32x4 {w == 0u ? (int)v : 0, w == 1u ? (int)v : 0, w == 2u ? (int)v : 0, w == 3u ? (int)v : 0};
}

} // namespace

} // namespace mvs
