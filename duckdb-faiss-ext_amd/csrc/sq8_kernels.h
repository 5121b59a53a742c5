// csrc/sq8_kernels.h -- what the kinds that hold 8-bit scalar-quantised rows share (csrc/sq.hip "SQ8" / "IVF<n>,SQ8", csrc/hnsw.hip
// "HNSW<M>,SQ8"): the rounded f32 operations, the two-stage min / max of the training rows, the derivation of (vdiff, s, a) and the encoder.
// Every kernel here has internal linkage: each translation unit that includes the header gets its own instance.
//
// Every operation of the contract is one IEEE f32 operation rounded on its own (csrc/sq.hip explains why __fmul_rn and friends do not
// give that under contraction).  A translation unit may be compiled with contraction on, so every function that does arithmetic here opens
// its own "#pragma clang fp contract(off)" scope: its operations carry no contraction flag and stay what they are after inlining.
#pragma once
#include "index.h"

namespace mvs {

namespace {

constexpr int SQ_MINMAX_ROWS = 512; // rows one lane of the first min / max stage folds

// one IEEE f32 operation each
__device__ __forceinline__ float sq_add(float x, float y) {
#pragma clang fp contract(off)
	return x + y;
}
__device__ __forceinline__ float sq_sub(float x, float y) {
#pragma clang fp contract(off)
	return x - y;
}
__device__ __forceinline__ float sq_mul(float x, float y) {
#pragma clang fp contract(off)
	return x * y;
}
__device__ __forceinline__ float sq_div(float x, float y) { // (f32 division is correctly rounded in device code)
#pragma clang fp contract(off)
	return x / y;
}

// ---------------------------------------------------------------------------------------------- train
// y = x[r][k], or x[r][k] - cent[label[r]][k] (label != null; a row without a list keeps x, as in csrc/ivfpq.hip)
__device__ __forceinline__ float sq_row_value(const float *__restrict__ x, long long r, int k, int d, const long long *__restrict__ label,
                                              const float *__restrict__ cent, long long nlist) {
	const float v = x[r * d + k];
	if (!label)
		return v;
	const long long l = label[r];
	return l >= 0 && l < nlist ? sq_sub(v, cent[l * d + k]) : v;
}
// part [chunks][2][d]: min and max of component k over the chunk's SQ_MINMAX_ROWS rows; blockIdx.y = the chunk
__global__ __launch_bounds__(256) void sq8_minmax_kernel(const float *__restrict__ x, long long n, int d, const long long *__restrict__ label,
                                                         const float *__restrict__ cent, long long nlist, float *__restrict__ part) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= d)
		return;
	const long long r0 = (long long)blockIdx.y * SQ_MINMAX_ROWS;
	const long long r1 = r0 + SQ_MINMAX_ROWS < n ? r0 + SQ_MINMAX_ROWS : n;
	float mn = sq_row_value(x, r0, k, d, label, cent, nlist), mx = mn;
	for (long long r = r0 + 1; r < r1; ++r) {
		const float v = sq_row_value(x, r, k, d, label, cent, nlist);
		mn = v < mn ? v : mn;
		mx = v > mx ? v : mx;
	}
	part[((size_t)blockIdx.y * 2 + 0) * d + k] = mn;
	part[((size_t)blockIdx.y * 2 + 1) * d + k] = mx;
}
// run [2][d] = the range of the chunks (and of run as it stands, unless this is the first batch)
__global__ __launch_bounds__(256) void sq8_minmax_fold_kernel(const float *__restrict__ part, int chunks, int d, float *__restrict__ run, int first) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= d)
		return;
	float mn = first ? part[k] : run[k], mx = first ? part[d + k] : run[d + k];
	for (int c = 0; c < chunks; ++c) {
		const float a = part[((size_t)c * 2 + 0) * d + k], b = part[((size_t)c * 2 + 1) * d + k];
		mn = a < mn ? a : mn;
		mx = b > mx ? b : mx;
	}
	run[k] = mn;
	run[d + k] = mx;
}
// par [4][d]: vmin | vdiff | a | s.  from_range: par[1] holds vmax on entry
__global__ __launch_bounds__(256) void sq8_derive_kernel(float *__restrict__ par, int d, int from_range) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= d)
		return;
	const float vmin = par[k];
	const float vdiff = from_range ? sq_sub(par[d + k], vmin) : par[d + k];
	const float s = sq_div(vdiff, 255.0f);
	par[d + k] = vdiff;
	par[3 * d + k] = s;
	par[2 * d + k] = sq_add(vmin, sq_mul(0.5f, s));
}

// ---------------------------------------------------------------------------------------------- encode
__global__ __launch_bounds__(256) void sq8_encode_kernel(const float *__restrict__ x, long long n, int d, const long long *__restrict__ label,
                                                         const float *__restrict__ cent, long long nlist, const float *__restrict__ par,
                                                         unsigned char *__restrict__ codes, int pitch, long long row0) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n * d)
		return;
	const long long r = i / d;
	const int k = (int)(i - r * d);
	const float y = sq_row_value(x, r, k, d, label, cent, nlist);
	const float vdiff = par[d + k];
	int code = 0;
	if (vdiff != 0.f) {
		float xi = sq_div(sq_sub(y, par[k]), vdiff);
		xi = xi < 0.f ? 0.f : (xi > 1.f ? 1.f : xi);
		code = (int)sq_mul(255.0f, xi);
	}
	codes[(row0 + r) * pitch + k] = (unsigned char)code;
}

} // namespace

} // namespace mvs
