// csrc/pq_kernels.h -- what the product-quantised index kinds share (csrc/pq.hip "PQ<M>", csrc/ivfpq.hip "IVF<n>,PQ<M>"): the geometry of
// the LDS table layouts, the order keys, the selector test, the encoder and the range selection.  Every kernel here has internal linkage:
// each translation unit that includes the header gets its own instance (pq_select_kernel also serves csrc/coded_lists.hip).
#pragma once
#include "index.h"

#include <cfloat>

namespace mvs {

namespace {

constexpr int PQ_KSUB = 256;            // 8 bits per code
constexpr int PQ_MAX_M = 128;           // scalar layout: 128 KB of tables for one query
constexpr int PQ_MAX_K = 2048;
constexpr int PQ_SCAN_THREADS = 1024;   // 4 waves per SIMD: the LDS gathers need the occupancy (ds_read_b32 / b64 want ~4 waves per SIMD)
constexpr int PQ_ROWS_PER_WG = 8192;    // rows one scan workgroup walks = entries of a query's bucket = the first range
constexpr int PQ_TABLE_LDS = 128 << 10; // table bytes per workgroup (of the CU's 160 KB)
constexpr int PQ_MAX_GROUPS = 8;
constexpr int PQ_ENCODE_LDS_DSUB = 64;  // 256 x dsub codebook + 256 x dsub rows in LDS: 128 KB at dsub = 64
constexpr size_t PQ_TABLE_SCRATCH = (size_t)64 << 20;
constexpr size_t PQ_BUCKET_SCRATCH = (size_t)256 << 20;

inline int pq_width(int M) { // queries interleaved per table entry
	return M <= 32 ? 4 : (M <= 64 ? 2 : 1);
}
inline int pq_groups(int M) { // groups of `width` queries whose tables one workgroup holds
	const int g = PQ_TABLE_LDS / (M * pq_width(M) * PQ_KSUB * (int)sizeof(float));
	return g < 1 ? 1 : (g > PQ_MAX_GROUPS ? PQ_MAX_GROUPS : g);
}

__device__ __forceinline__ bool pq_sel_member(const SelectorDev &s, long long id) {
	if (s.kind == MVS_SEL_BITMAP) {
		const unsigned long long u = (unsigned long long)id;
		if ((u >> 3) >= (unsigned long long)s.nbytes)
			return false;
		return (s.bitmap[u >> 3] >> (u & 7)) & 1;
	}
	if (s.kind == MVS_SEL_BATCH) {
		long long lo = 0, hi = s.nids;
		while (lo < hi) {
			const long long mid = (lo + hi) >> 1;
			if (s.sorted_ids[mid] < id)
				lo = mid + 1;
			else
				hi = mid;
		}
		return lo < s.nids && s.sorted_ids[lo] == id;
	}
	return true;
}
// order key of a value: smaller key = better entry (L2: the value's ascending order; inner product: descending)
__device__ __forceinline__ unsigned pq_key(float v, int descending) {
	const unsigned b = __float_as_uint(v);
	const unsigned a = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
	return descending ? ~a : a;
}
__device__ __forceinline__ float pq_unkey(unsigned key, int descending) {
	const unsigned a = descending ? ~key : key;
	return __uint_as_float((a >> 31) ? (a ^ 0x80000000u) : ~a);
}
// The ADMISSION RULE of the scanning coded kinds (PQ<M>, SQ8, IVF<n>,PQ<M>, IVF<n>,SQ8) = FAISS's heap: the k-list starts full of
// (neutral, -1), neutral = FLT_MAX (L2) / -FLT_MAX (inner product), and a value enters only if it is STRICTLY better than the list's
// worst -- a float comparison, false for NaN.  So a NaN is never a result, and neither is a value not strictly better than the
// neutral element: +inf (an overflowed L2 sum) and FLT_MAX itself under L2, -inf and -FLT_MAX under inner product.  Such slots print
// as (-1, neutral).  Here the rule is the bound an OPEN list starts with and the test a scan makes against a bound:
//   PQ_OPEN_BOUND    pq_key(FLT_MAX, 0) == pq_key(-FLT_MAX, 1) == 0xFF7FFFFF: "better than the bound" is "strictly better than neutral"
//   pq_beats         the test itself, made on the VALUE, as FAISS makes it: the bound's key is turned back into its float once per query
//                    (pq_bound_value) and a row's value is compared with it -- one compare (after one sign flip under inner product),
//                    false for a NaN of either sign, and nothing of the key is formed for a row that does not enter.  Testing the KEY
//                    would order a NaN by its bit pattern: one sign's NaN is the best key of each metric.  Key order and value order
//                    agree on everything else but +0.0 against -0.0, and no chain here ends in -0.0 (they start from +0.0)
// (csrc/refine.hip re-ranks with pq_key itself: FAISS's reorder_2_heaps is another contract.)
constexpr unsigned PQ_OPEN_BOUND = 0xFF7FFFFFu;
__device__ __forceinline__ unsigned pq_sign_mask(int descending) {
	return descending ? 0x80000000u : 0u;
}
// the bound a query's key `thr` stands for, on the ascending side (negated under inner product); thr == 0, "no key is below it", gives
// a NaN, which no value beats
__device__ __forceinline__ float pq_bound_value(unsigned thr, int descending) {
	return __uint_as_float(__float_as_uint(pq_unkey(thr, descending)) ^ pq_sign_mask(descending));
}
__device__ __forceinline__ bool pq_beats(float v, float bound_value, unsigned sign_mask) {
	return __uint_as_float(__float_as_uint(v) ^ sign_mask) < bound_value;
}
// the bounds of a chunk's n queries before its first range
inline void pq_open_bounds(unsigned *thr, size_t n, hipStream_t st) {
	MVS_HIP(hipMemsetD32Async((hipDeviceptr_t)thr, static_cast<int>(PQ_OPEN_BOUND), n, st)); // (the 32-bit pattern; the API takes it as int)
}

// ---------------------------------------------------------------------------------------------- encode
__global__ __launch_bounds__(256) void pq_encode_kernel(const float *__restrict__ x, long long n, int d, int dsub, const float *__restrict__ cb,
                                                        unsigned char *__restrict__ codes, int pitch, long long row0, int in_lds) {
	extern __shared__ float pq_enc_lds[];
	const int m = blockIdx.y, tid = threadIdx.x;
	const long long blk0 = (long long)blockIdx.x * 256, r = blk0 + tid;
	const float *cbm = cb + (size_t)m * PQ_KSUB * dsub;
	const float *c, *xs;
	int xstride;
	if (in_lds) {
		float *cs = pq_enc_lds, *xt = pq_enc_lds + PQ_KSUB * dsub; // xt [k][lane]: a lane's reads hit its own bank
		for (int i = tid; i < PQ_KSUB * dsub; i += 256)
			cs[i] = cbm[i];
		for (int i = tid; i < 256 * dsub; i += 256) {
			const int rr = i / dsub, k = i - rr * dsub;
			const long long row = blk0 + rr;
			xt[k * 256 + rr] = row < n ? x[row * d + (long long)m * dsub + k] : 0.f;
		}
		__syncthreads();
		c = cs;
		xs = xt + tid;
		xstride = 256;
	} else {
		c = cbm;
		xs = x + (r < n ? r : n - 1) * d + (long long)m * dsub;
		xstride = 1;
	}
	float best = 0.f;
	int bj = 0;
	for (int j = 0; j < PQ_KSUB; ++j) {
		const float *cj = c + j * dsub; // (the same address in every lane: an LDS broadcast)
		float acc = 0.f;
		for (int k = 0; k < dsub; ++k) {
			const float t = xs[k * xstride] - cj[k];
			acc = fmaf(t, t, acc);
		}
		if (j == 0 || acc < best) {
			best = acc;
			bj = j;
		}
	}
	if (r < n)
		codes[(row0 + r) * pitch + m] = (unsigned char)bj;
}

// ---------------------------------------------------------------------------------------------- table entries
// ---------------------------------------------------------------------------------------------- scan
template <int W>
struct PqEntry;
template <>
struct PqEntry<4> {
	typedef float4 type;
	static __device__ __forceinline__ void add(float *acc, const float4 &t) {
		acc[0] += t.x, acc[1] += t.y, acc[2] += t.z, acc[3] += t.w;
	}
};
template <>
struct PqEntry<2> {
	typedef float2 type;
	static __device__ __forceinline__ void add(float *acc, const float2 &t) {
		acc[0] += t.x, acc[1] += t.y;
	}
};
template <>
struct PqEntry<1> {
	typedef float type;
	static __device__ __forceinline__ void add(float *acc, const float &t) {
		acc[0] += t;
	}
};

// ---------------------------------------------------------------------------------------------- select
// list [nqc][k] sorted keys, len [nqc]; bucket [nqc][R], cnt [nqc] (<= R: the caller has checked the overflow flag)
__global__ __launch_bounds__(1024) void pq_select_kernel(unsigned long long *__restrict__ list, int *__restrict__ len, int k,
                                                         const unsigned long long *__restrict__ bucket, unsigned *__restrict__ cnt,
                                                         unsigned *__restrict__ thr) {
	extern __shared__ unsigned long long pq_sel_lds[];
	const long long q = blockIdx.x;
	const int tid = threadIdx.x, nt = blockDim.x;
	const int nl = len[q], nb = (int)cnt[q], total = nl + nb;
	if (nb == 0)
		return; // (the list and its bound stand)
	int P = 1;
	while (P < total)
		P <<= 1;
	for (int i = tid; i < P; i += nt)
		pq_sel_lds[i] = i < nl ? list[q * k + i] : (i < total ? bucket[(size_t)q * PQ_ROWS_PER_WG + (i - nl)] : ~0ull);
	__syncthreads();
	for (int kk = 2; kk <= P; kk <<= 1)
		for (int j = kk >> 1; j > 0; j >>= 1) {
			for (int i = tid; i < P; i += nt) {
				const int p = i ^ j;
				if (p > i) {
					const unsigned long long a = pq_sel_lds[i], b = pq_sel_lds[p];
					if ((a > b) == ((i & kk) == 0)) {
						pq_sel_lds[i] = b;
						pq_sel_lds[p] = a;
					}
				}
			}
			__syncthreads();
		}
	const int keep = total < k ? total : k;
	for (int i = tid; i < keep; i += nt)
		list[q * k + i] = pq_sel_lds[i];
	if (tid == 0) {
		len[q] = keep;
		cnt[q] = 0u;
		if (keep == k)
			thr[q] = (unsigned)(pq_sel_lds[k - 1] >> 32);
	}
}

} // namespace

} // namespace mvs
