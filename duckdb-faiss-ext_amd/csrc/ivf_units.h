// csrc/ivf_units.h -- what the index kinds with coded inverted lists share (csrc/ivfpq.hip "IVF<n>,PQ<M>", csrc/sq.hip "SQ8" /
// "IVF<n>,SQ8"): the gather into the list-sorted code view, the ordinal bases and the counting sort that groups the (query, rank) pairs
// of one unit by list.  Every kernel here has internal linkage: each translation unit that includes the header gets its own instance.
#pragma once
#include "index.h"

namespace mvs {

namespace {

// out[i] = codes[perm[i]], rows of `pitch` bytes moved as 16-byte words
__global__ __launch_bounds__(256) void ivfpq_gather_codes_kernel(const uint4 *__restrict__ codes, const int *__restrict__ perm, long long n, int words,
                                                                 uint4 *__restrict__ out) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n * words)
		return;
	const long long r = i / words;
	const int w = (int)(i - r * words);
	out[i] = codes[(long long)perm[r] * words + w];
}

// ---------------------------------------------------------------------------------------------- ordinals
// pref [nq][np + 1]: rows of the lists probed at ranks below r (a -1 probe has none)
__global__ __launch_bounds__(256) void ivfpq_prefix_kernel(const long long *__restrict__ cI, long long nq, int np, const long long *__restrict__ list_off,
                                                           long long nlist, unsigned *__restrict__ pref) {
	const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= nq)
		return;
	unsigned acc = 0;
	for (int r = 0; r < np; ++r) {
		pref[q * (np + 1) + r] = acc;
		const long long l = cI[q * np + r];
		if (l >= 0 && l < nlist)
			acc += (unsigned)(list_off[l + 1] - list_off[l]);
	}
	pref[q * (np + 1) + np] = acc;
}

// ---------------------------------------------------------------------------------------------- grouping
// the pairs (query of the chunk, rank in [ra, rb)) whose list has rows at or beyond position p0, counted per list
__global__ __launch_bounds__(256) void ivfpq_count_kernel(const long long *__restrict__ cI, long long nqc, int np, int ra, int rb,
                                                          const long long *__restrict__ list_off, long long nlist, long long p0, int *__restrict__ cnt) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	const int span = rb - ra;
	if (i >= nqc * span)
		return;
	const long long q = i / span;
	const int r = ra + (int)(i - q * span);
	const long long l = cI[q * np + r];
	if (l >= 0 && l < nlist && list_off[l + 1] - list_off[l] > p0)
		atomicAdd(&cnt[l], 1);
}
// poff [nlist + 1]: first pair of every list; goff [nlist + 1]: first pair GROUP (<= Q pairs) of every list.  One workgroup.
__global__ __launch_bounds__(1024) void ivfpq_offsets_kernel(const int *__restrict__ cnt, int nlist, int Q, int *__restrict__ poff, int *__restrict__ goff) {
	__shared__ int sp[1024], sg[1024];
	const int tid = threadIdx.x;
	const int per = (nlist + 1023) / 1024;
	const int l0 = tid * per, l1 = l0 + per < nlist ? l0 + per : nlist;
	int ap = 0, ag = 0;
	for (int l = l0; l < l1; ++l) {
		ap += cnt[l];
		ag += (cnt[l] + Q - 1) / Q;
	}
	sp[tid] = ap, sg[tid] = ag;
	__syncthreads();
	for (int s = 1; s < 1024; s <<= 1) { // inclusive scan of the 1024 partial sums
		const int vp = tid >= s ? sp[tid - s] : 0, vg = tid >= s ? sg[tid - s] : 0;
		__syncthreads();
		sp[tid] += vp, sg[tid] += vg;
		__syncthreads();
	}
	int bp = sp[tid] - ap, bg = sg[tid] - ag;
	for (int l = l0; l < l1; ++l) {
		poff[l] = bp, goff[l] = bg;
		bp += cnt[l];
		bg += (cnt[l] + Q - 1) / Q;
	}
	if (tid == 1023)
		poff[nlist] = sp[1023], goff[nlist] = sg[1023];
}
__global__ __launch_bounds__(256) void ivfpq_scatter_kernel(const long long *__restrict__ cI, long long nqc, int np, int ra, int rb,
                                                            const long long *__restrict__ list_off, long long nlist, long long p0,
                                                            const int *__restrict__ poff, int *__restrict__ cur, int2 *__restrict__ pairs) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	const int span = rb - ra;
	if (i >= nqc * span)
		return;
	const long long q = i / span;
	const int r = ra + (int)(i - q * span);
	const long long l = cI[q * np + r];
	if (l >= 0 && l < nlist && list_off[l + 1] - list_off[l] > p0)
		pairs[poff[l] + atomicAdd(&cur[l], 1)] = make_int2((int)q, r);
}

} // namespace

} // namespace mvs
