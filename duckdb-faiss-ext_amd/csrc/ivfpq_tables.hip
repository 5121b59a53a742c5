// csrc/ivfpq_tables.hip -- the two table kernels of "IVF<n>,PQ<M>"'s option ivfpq_precomputed_table (include/mi355_faiss.h
// "precomputed tables").  The table entry of a (query, list) pair splits into a part that depends on the list alone and
// a part that depends on the query alone; csrc/ivfpq.hip's scan joins them with one fmaf per entry instead of running a chain per entry.
//
//   p = codebook[m][j], x_m / c_m = sub-vector m of the query / of the list's centroid; every chain is acc = fmaf(a_k, b_k, acc), k ascending from +0
//   ivfpq_list_table_kernel    L[l][m][j] = fmaf(2, <c_m, p>, <p, p>)   once per (centroids, codebooks), L2 only; plain lanes
//   ivfpq_query_table_kernel   S[q][m][j] = <x_m, p>                    once per query chunk; v_mfma_f32_32x32x2_f32, which IS that chain
//                              (csrc/flat_mfma.hip "arithmetic contract", tests/test_mfma_model_gpu.py)
//
// Every operation is one IEEE f32 operation rounded on its own: the unit is compiled with contraction off (as csrc/sq.hip).
#include "ivfpq_tables.h"

#pragma clang fp contract(off)

namespace mvs {

namespace {

constexpr int PQ_KSUB = 256; // entries of a codebook (csrc/pq_kernels.h, whose kernels this unit does not need)

// ---------------------------------------------------------------------------------------------- per list
// workgroup = (list l, sub-space m); lane j takes codebook entry j; the centroid's sub-vector is staged in LDS (every lane reads the
// same word: a broadcast).  The codebook is read with a stride of dsub floats between lanes -- off the hot path
__global__ __launch_bounds__(PQ_KSUB) void ivfpq_list_table_kernel(const float *__restrict__ cent, const float *__restrict__ cb, int d, int M, int dsub,
                                                                   float *__restrict__ L) {
	extern __shared__ float lt_c[]; // [dsub]
	const int l = blockIdx.x, m = blockIdx.y, j = threadIdx.x;
	for (int k = j; k < dsub; k += PQ_KSUB)
		lt_c[k] = cent[(size_t)l * d + (size_t)m * dsub + k];
	__syncthreads();
	const float *p = cb + ((size_t)m * PQ_KSUB + j) * dsub;
	float cp = 0.f, pp = 0.f;
	for (int k = 0; k < dsub; ++k) {
		const float pk = p[k];
		cp = fmaf(lt_c[k], pk, cp);
		pp = fmaf(pk, pk, pp);
	}
	L[((size_t)l * M + m) * PQ_KSUB + j] = fmaf(2.f, cp, pp);
}

// ---------------------------------------------------------------------------------------------- per query
// Block-diagonal product: for sub-space m, S[:, m, :] = X[:, m dsub .. (m+1) dsub) . codebook[m]^T, [nqc x dsub] . [dsub x 256].
// Workgroup = (64 queries, ONE sub-space), 4 waves.  The sub-space's codebook -- 256 entries x <= 32 columns at a time -- and the
// queries' columns are staged in LDS once; wave w takes the two 32-entry tiles 2 w, 2 w + 1 as A operands and the two 32-query tiles as
// B operands: four 32x32 accumulators, every LDS word read feeds two MFMAs.  D[i][j] lands with the query j = lane & 31 on the lane and
// the entries i = 8 (e >> 2) + 4 (lane >> 5) + (e & 3) in its registers: four consecutive entries per float4 store, 256 consecutive
// floats per (query, m) in S, which is how the scan reads it.  dsub goes in steps of 2; an odd tail is zero-padded on both operands,
// fma(0, 0, acc) = acc.  Pitch 34 words: the 32 lanes of a half read 32 distinct even (odd) banks.
constexpr int QT_THREADS = 256;
constexpr int QT_NQ = IVFPQ_QT_QUERIES;
constexpr int QT_KC = 32;           // columns of the sub-space staged at a time (dsub <= 32: one pass)
constexpr int QT_PITCH = QT_KC + 2; // words per staged row
typedef float qt_f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(QT_THREADS) void ivfpq_query_table_kernel(const float *__restrict__ xq, long long nqc, int d, int M, int dsub,
                                                                       const float *__restrict__ cb, float *__restrict__ S) {
	__shared__ float cs[PQ_KSUB * QT_PITCH]; // codebook entries [256][kc]
	__shared__ float xs[QT_NQ * QT_PITCH];   // queries [64][kc]
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int h = lane >> 5, c = lane & 31;
	const long long q0 = (long long)blockIdx.x * QT_NQ;
	const int m = blockIdx.y;
	const float *cbm = cb + (size_t)m * PQ_KSUB * dsub;
	qt_f32x16 acc[2][2]; // [entry tile][query tile]
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int b = 0; b < 2; ++b)
#pragma unroll
			for (int e = 0; e < 16; ++e)
				acc[t][b][e] = 0.f;
	const float *aw = cs + (wave * 64 + c) * QT_PITCH + h; // A operand: entry (lane & 31) of the tile, column 2 s + (lane >> 5)
	const float *bw = xs + c * QT_PITCH + h;               // B operand: query (lane & 31) of the tile, the same column
	for (int k0 = 0; k0 < dsub; k0 += QT_KC) { // (uniform trip counts: every lane reaches every barrier)
		const int kc = dsub - k0 < QT_KC ? dsub - k0 : QT_KC, kce = (kc + 1) & ~1;
		if (k0 > 0)
			__syncthreads(); // (the previous columns have been read)
		for (int i = tid; i < PQ_KSUB * kce; i += QT_THREADS) {
			const int j = i / kce, k = i - j * kce;
			cs[j * QT_PITCH + k] = k < kc ? cbm[(size_t)j * dsub + k0 + k] : 0.f;
		}
		for (int i = tid; i < QT_NQ * kce; i += QT_THREADS) {
			const int qi = i / kce, k = i - qi * kce;
			xs[qi * QT_PITCH + k] = k < kc && q0 + qi < nqc ? xq[(size_t)(q0 + qi) * d + (size_t)m * dsub + k0 + k] : 0.f;
		}
		__syncthreads();
		for (int s = 0; s < kce / 2; ++s) {
			const float a0 = aw[2 * s], a1 = aw[32 * QT_PITCH + 2 * s];
			const float b0 = bw[2 * s], b1 = bw[32 * QT_PITCH + 2 * s];
			acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
			acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
			acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
			acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
		}
	}
#pragma unroll
	for (int b = 0; b < 2; ++b) {
		const long long q = q0 + b * 32 + c;
		if (q >= nqc)
			continue;
		float *Sq = S + ((size_t)q * M + m) * PQ_KSUB;
#pragma unroll
		for (int t = 0; t < 2; ++t)
#pragma unroll
			for (int g = 0; g < 4; ++g) {
				const int i = (wave * 2 + t) * 32 + 8 * g + 4 * h;
				*reinterpret_cast<float4 *>(Sq + i) = make_float4(acc[t][b][4 * g], acc[t][b][4 * g + 1], acc[t][b][4 * g + 2], acc[t][b][4 * g + 3]);
			}
	}
}

} // namespace

void launch_ivfpq_list_table(const float *d_cent, const float *d_cb, int64_t nlist, int d, int M, float *d_L, hipStream_t st) {
	const int dsub = d / M;
	const size_t lds = (size_t)dsub * sizeof(float);
	if (lds > (48u << 10))
		throw_faiss("mvs::launch_ivfpq_list_table", __FILE__, "ivfpq_precomputed_table serves sub-vectors of at most %d components (d / M = %d)",
		            (int)((48u << 10) / sizeof(float)), dsub);
	hipLaunchKernelGGL(ivfpq_list_table_kernel, dim3((unsigned)nlist, (unsigned)M), dim3(PQ_KSUB), lds, st, d_cent, d_cb, d, M, dsub, d_L);
	MVS_HIP(hipGetLastError());
}
void launch_ivfpq_query_table(const float *d_xq, int64_t nqc, int d, int M, const float *d_cb, float *d_S, hipStream_t st) {
	hipLaunchKernelGGL(ivfpq_query_table_kernel, dim3((unsigned)((nqc + QT_NQ - 1) / QT_NQ), (unsigned)M), dim3(QT_THREADS), 0, st, d_xq,
	                   (long long)nqc, d, M, d / M, d_cb, d_S);
	MVS_HIP(hipGetLastError());
}

} // namespace mvs
