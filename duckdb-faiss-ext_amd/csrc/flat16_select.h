// csrc/flat16_select.h -- what the two fp16 scans share: half-precision Flat (csrc/flat_f16.hip) and bfKnn over a caller's fp16 matrix
// (csrc/bf_knn.hip).  The arithmetic of a score's test, the record stream, the per-generation merge kernels and the norm chain over a
// fragment-major store, exactly as csrc/flat_f16.hip held them before the split: both translation units compile these lines, so a bfKnn
// over rows h gives the bits of a half-precision Flat index over the same h.  Everything is in an unnamed namespace: each translation unit
// has its own copy of the kernels.  Include it with contraction off (#pragma clang fp contract(off), as csrc/sq.hip explains).
#pragma once
#include "index.h"
#include "pq_kernels.h"

#include <hip/hip_fp16.h>

#include <algorithm>

namespace mvs {

namespace {

constexpr int F16_MAX_D = 2048, F16_MAX_K = 2048;
constexpr int F16_TILE = 64;                          // rows of a tile: four 16-row MFMA operands
constexpr int64_t F16_QCHUNK = 16384;                 // queries per pass
constexpr int64_t F16_MAX_STREAM = (int64_t)1 << 26;  // records of the largest stream (12 bytes each); a generation that needs more is halved
constexpr int64_t F16_GROWTH = 4;                     // a generation ends at 4 x the rows scanned before it
constexpr unsigned long long F16_OPEN = ~0ull;        // no bound yet / an empty list entry: above every key a row can have
constexpr unsigned MAX_BLOCKS = 1u << 20;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

unsigned grid_for(long long n, int per_block = 256) {
	return (unsigned)std::max<long long>(1, std::min<long long>((n + per_block - 1) / per_block, MAX_BLOCKS));
}

__device__ __forceinline__ float f16_lo(unsigned w) {
	return __half2float(__ushort_as_half((unsigned short)(w & 0xFFFFu)));
}
__device__ __forceinline__ float f16_hi(unsigned w) {
	return __half2float(__ushort_as_half((unsigned short)(w >> 16)));
}
// out[row - row0] = the chain acc = fmaf(v, v, acc) over the decoded halves of `row`, k ascending from +0 (the padding's zeros leave it
// as it is).  One thread per row
__global__ __launch_bounds__(256) void flat16_norm_kernel(const uint4 *__restrict__ words, int S, long long row0, long long n, float *__restrict__ out) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
		const long long row = row0 + i;
		const uint4 *wp = words + (row >> 4) * S * 64 + (row & 15);
		float acc = 0.f;
		for (int s = 0; s < S; ++s)
			for (int g = 0; g < 4; ++g) {
				const uint4 w = wp[s * 64 + g * 16];
				const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
				for (int e = 0; e < 4; ++e) {
					const float lo = f16_lo(u[e]), hi = f16_hi(u[e]);
					acc = fmaf(lo, lo, acc);
					acc = fmaf(hi, hi, acc);
				}
			}
		out[i] = acc;
	}
}

// ---------------------------------------------------------------------------------------------- scan
struct F16Scan {
	const uint4 *rows;   // the store
	const float *norms;  // [cap] n_i
	const uint4 *qf;     // the chunk's queries in the store's layout, padded with zero rows to a multiple of 64
	const float *qn;     // [nq padded] m_q
	const unsigned long long *T;     // [nq padded] bounds; a padded query's bound is 0: nothing is below it
	const unsigned long long *allow; // [tiles] or null
	long long n, tile0, tile1;
	int nq, S, l2, nqw; // nqw: waves of a workgroup that take different query groups (d <= 128)
	unsigned long long *keys;
	uint32_t *recq;
	unsigned long long *cnt;
	long long cap;
};

// The admitted lanes of a wave take consecutive stream slots: one atomic per wave.  A record beyond the capacity is counted, not written
__device__ __forceinline__ long long f16_stream_slot(bool adm, unsigned long long *cnt, int lane) {
	const unsigned long long m = __ballot(adm);
	if (!m)
		return -1;
	const int leader = __ffsll((long long)m) - 1;
	unsigned long long base = 0;
	if (lane == leader)
		base = atomicAdd(cnt, (unsigned long long)__popcll(m));
	base = __shfl(base, leader);
	return adm ? (long long)(base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull))) : -1;
}

// what a lane keeps of its query for the launch: the bound's pair, and the bound's score on the ascending side for the cheap test (an
// open bound passes every number; a padded query's 0 gives a NaN, which nothing passes)
struct F16Bound {
	unsigned long long t;
	float tb, mq;
};
__device__ __forceinline__ F16Bound f16_bound(const F16Scan &a, int q) {
	F16Bound b;
	b.t = a.T[q];
	const unsigned thi = (unsigned)(b.t >> 32);
	b.tb = thi == 0xFFFFFFFFu ? __uint_as_float(0x7F800000u) : pq_bound_value(thi, a.l2 ? 0 : 1);
	b.mq = a.qn[q];
	return b;
}

// the scores of (16 rows 16 i + 4 g .. + 3 of `tile`) x (query q): score, cheap test on the value, then the rule and the pair inside
__device__ __forceinline__ void f16_test4(const F16Scan &a, const f32x4 &acc, const F16Bound &b, const float4 &nr, long long row4, int q,
                                          unsigned long long aw, int bit4, int lane) {
	const unsigned mask = pq_sign_mask(a.l2 ? 0 : 1);
	const float nrm[4] = {nr.x, nr.y, nr.z, nr.w};
	float v[4];
	bool hit = false;
#pragma unroll
	for (int r = 0; r < 4; ++r) {
		float s = acc[r];
		if (a.l2) {
			s = fmaf(-2.f, s, b.mq + nrm[r]);
			s = s < 0.f ? 0.f : s; // FAISS's BLAS-path clamp: a NaN stays a NaN
		}
		v[r] = s;
		hit = hit || __uint_as_float(__float_as_uint(s) ^ mask) <= b.tb;
	}
	if (!__ballot(hit))
		return;
	const float neutral = pq_bound_value(PQ_OPEN_BOUND, a.l2 ? 0 : 1);
#pragma unroll
	for (int r = 0; r < 4; ++r) {
		const long long row = row4 + r;
		const bool ok = row < a.n && ((aw >> (bit4 + r)) & 1ull);
		const unsigned long long key = ((unsigned long long)pq_key(v[r], a.l2 ? 0 : 1) << 32) | (unsigned long long)(unsigned)row;
		const bool adm = ok && pq_beats(v[r], neutral, mask) && key < b.t;
		const long long slot = f16_stream_slot(adm, a.cnt, lane);
		if (adm && slot < a.cap) {
			a.keys[slot] = key;
			a.recq[slot] = (uint32_t)q;
		}
	}
}

// ---------------------------------------------------------------------------------------------- records -> lists
__global__ __launch_bounds__(256) void flat16_hist_kernel(const uint32_t *__restrict__ recq, long long n, unsigned *__restrict__ qcnt) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
		atomicAdd(&qcnt[recq[i]], 1u);
}
// records into their query's segment [qoff[q], qoff[q] + qcnt[q]); the order inside a segment is the atomics', the select sorts it away
__global__ __launch_bounds__(256) void flat16_scatter_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ recq, long long n,
                                                             const unsigned *__restrict__ qoff, unsigned *__restrict__ qfill,
                                                             unsigned long long *__restrict__ seg) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
		const uint32_t q = recq[i];
		seg[qoff[q] + atomicAdd(&qfill[q], 1u)] = keys[i];
	}
}
// One workgroup per query: its k best pairs so far and its segment's records, K2 at a time, through a bitonic sort of 2 K2 keys in LDS (K2 a
// power of two >= k); the K2 smallest stay.  The keys of one query are distinct, so the outcome is its k smallest pairs in order, and the
// k-th is the bound of the next generation
__global__ __launch_bounds__(256) void flat16_select_kernel(const unsigned long long *__restrict__ seg, const unsigned *__restrict__ qoff,
                                                            const unsigned *__restrict__ qcnt, int k, int K2, unsigned long long *__restrict__ best,
                                                            unsigned long long *__restrict__ T) {
	extern __shared__ unsigned long long f16_sel[];
	const int q = blockIdx.x, tid = threadIdx.x;
	const unsigned len = qcnt[q];
	if (len == 0)
		return;
	const unsigned long long *sp = seg + qoff[q];
	unsigned long long *bq = best + (size_t)q * k;
	const int S2 = 2 * K2;
	for (int i = tid; i < K2; i += 256)
		f16_sel[i] = i < k ? bq[i] : F16_OPEN;
	for (unsigned c0 = 0; c0 < len; c0 += (unsigned)K2) {
		for (int i = tid; i < K2; i += 256)
			f16_sel[K2 + i] = c0 + (unsigned)i < len ? sp[c0 + (unsigned)i] : F16_OPEN;
		__syncthreads();
		for (int size = 2; size <= S2; size <<= 1)
			for (int stride = size >> 1; stride > 0; stride >>= 1) {
				for (int i = tid; i < S2 / 2; i += 256) {
					const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
					const bool up = (lo & size) == 0;
					const unsigned long long x = f16_sel[lo], y = f16_sel[hi];
					if ((x > y) == up) {
						f16_sel[lo] = y;
						f16_sel[hi] = x;
					}
				}
				__syncthreads();
			}
	}
	for (int i = tid; i < k; i += 256)
		bq[i] = f16_sel[i];
	if (tid == 0)
		T[q] = f16_sel[k - 1];
}
__global__ __launch_bounds__(256) void flat16_fill_kernel(unsigned long long *__restrict__ p, long long n, unsigned long long v) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
		p[i] = v;
}
// best pairs -> (score, label); an open entry is the padding (+-FLT_MAX, -1)
__global__ __launch_bounds__(256) void flat16_emit_kernel(const unsigned long long *__restrict__ best, long long total, int descending,
                                                          const long long *__restrict__ ids, long long label_offset, float *__restrict__ D,
                                                          long long *__restrict__ I) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const unsigned long long key = best ? best[i] : F16_OPEN;
		if (key == F16_OPEN) {
			D[i] = descending ? -FLT_MAX : FLT_MAX;
			I[i] = -1;
		} else {
			const long long row = (long long)(unsigned)key;
			D[i] = pq_unkey((unsigned)(key >> 32), descending);
			I[i] = ids ? ids[row] : row + label_offset;
		}
	}
}

} // namespace

} // namespace mvs
