// csrc/pretransform.hip -- "<t1>,...,<tn>,<sub>" (faiss::IndexPreTransform, MVS_KIND_PRETRANSFORM): a chain of vector transforms -- PCA<o>,
// PCAW<o>, L2norm from the factory; any plain linear transform from a file or mvs_index_pretransform_set_linear -- in front of ONE owned
// sub-index of any other kind at the chain's output dimension.  Rows and queries are transformed on the device, then forwarded.
//
// Contract (include/mi355_faiss.h "pre-transform indexes"):
//   linear  y[j] = (acc = fmaf(x[k], A[j][k], acc), k ascending from +0) + b[j]; the bias is ONE f32 addition after the chain and absent
//           without a bias
//   L2norm  nr = (acc = fmaf(x[k], x[k], acc) from +0); nr > 0: y[k] = x[k] * (1.0f / sqrtf(nr)), else the row is copied (fvec_renorm_L2)
//   PCA     mean and covariance in f64 on the device (fixed row segments, fixed reduction order), eigenpairs by a one-sided (Hestenes) Jacobi
//           method in f64 on the device with a round-robin pair order, then order / sign / the one rounding to f32 on the host
//
// pretransform_apply_kernel<NT, VEC>: v_mfma_f32_32x32x2_f32, which is bit for bit a k-ordered fmaf chain (csrc/flat_mfma.hip).
//   workgroup  256 lanes = 4 waves; a block of 128 rows of x (M side, 32 rows a wave) against 32 NT outputs j (N side), NT = 1 | 2 | 4 | 8
//   k          streamed in chunks of 32 in ascending order: the chunk of x [128][32] and of A [32 NT][32] go to LDS (row pitch 34 floats:
//              lane (row r, half h) reads word 34 r + 2 s + h, 64 distinct banks), zero filled past n, d_out and d_in: fma(0, 0, acc) = acc
//              the NEXT chunk's global loads are issued into registers before the MFMAs of this one and stored to LDS after them
//   step s     every lane reads ONE x word and NT A words (ds_read_b32) and issues NT MFMAs into NT accumulator tiles
//   epilogue   D[i][j]: j on the lane (lane & 31), 16 rows i in the registers; + b[j]; 32 lanes write 128 contiguous bytes of a row of y
//   traffic    x is read from HBM once while d_out <= 256 (one pass per 256 outputs otherwise) and y written once; A comes from L2, d_out
//              d_in 4 bytes per workgroup.  VEC: rows of x are 16-byte aligned (d_in % 4 == 0 and the pointer), loads are 16 bytes a lane
#include "index.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#pragma clang fp contract(off)

namespace mvs {

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_BM = 128;                           // rows of x per workgroup
constexpr int PT_KC = 32;                            // k per staged chunk
constexpr int PT_PITCH = PT_KC + 2;                  // LDS row pitch in floats
constexpr size_t PT_WS_BYTES = (size_t)256 << 20;    // workspace of one add chunk
constexpr int PT_MAX_D = 2048, PT_MAX_CHAIN = 4;
constexpr double PT_JACOBI_TOL = 1e-12;
constexpr int PT_JACOBI_SWEEPS = 30;

typedef float pt_f32x16 __attribute__((ext_vector_type(16)));

struct ApplyArgs {
	const float *x; // [n][d_in]
	const float *A; // [d_out][d_in]
	const float *b; // [d_out] or null
	float *y;       // [n][d_out]
	long long n;
	int d_in, d_out;
};

// rows [row0, row0 + ROWS) x columns [k0, k0 + 32) of src [nrows][ld] into the lane's registers, zeros outside nrows / kc: pt_load issues the
// global loads, pt_store puts them into dst [ROWS][PT_PITCH] -- between the two the previous chunk's MFMAs run
template <int ROWS, bool VEC>
__device__ __forceinline__ void pt_load(float (&r)[ROWS * 32 / PT_THREADS], const float *src, long long row0, long long nrows, int ld, int k0, int kc,
                                        int tid) {
	if (VEC) { // (kc is a multiple of 4 here)
#pragma unroll
		for (int it = 0; it < ROWS * 8 / PT_THREADS; ++it) {
			const int f = it * PT_THREADS + tid, row = f >> 3, p = (f & 7) * 4;
			float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
			if (row0 + row < nrows && p < kc)
				v = *reinterpret_cast<const float4 *>(src + (size_t)(row0 + row) * ld + k0 + p);
			r[4 * it] = v.x, r[4 * it + 1] = v.y, r[4 * it + 2] = v.z, r[4 * it + 3] = v.w;
		}
	} else {
#pragma unroll
		for (int it = 0; it < ROWS * 32 / PT_THREADS; ++it) {
			const int f = it * PT_THREADS + tid, row = f >> 5, p = f & 31;
			r[it] = row0 + row < nrows && p < kc ? src[(size_t)(row0 + row) * ld + k0 + p] : 0.f;
		}
	}
}
template <int ROWS, bool VEC>
__device__ __forceinline__ void pt_store(float *dst, const float (&r)[ROWS * 32 / PT_THREADS], int tid) {
	if (VEC) {
#pragma unroll
		for (int it = 0; it < ROWS * 8 / PT_THREADS; ++it) {
			const int f = it * PT_THREADS + tid, row = f >> 3, p = (f & 7) * 4;
			float2 *o = reinterpret_cast<float2 *>(dst + row * PT_PITCH + p); // (pitch 34: 8-byte aligned)
			o[0] = make_float2(r[4 * it], r[4 * it + 1]);
			o[1] = make_float2(r[4 * it + 2], r[4 * it + 3]);
		}
	} else {
#pragma unroll
		for (int it = 0; it < ROWS * 32 / PT_THREADS; ++it) {
			const int f = it * PT_THREADS + tid;
			dst[(f >> 5) * PT_PITCH + (f & 31)] = r[it];
		}
	}
}

template <int NT, bool VEC>
__global__ __launch_bounds__(PT_THREADS, NT == 8 ? 1 : 2) void pretransform_apply_kernel(const ApplyArgs a) {
	__shared__ __attribute__((aligned(16))) float xs[PT_BM * PT_PITCH];
	__shared__ __attribute__((aligned(16))) float as[NT * 32 * PT_PITCH];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int h = lane >> 5, c = lane & 31;
	const long long row0 = (long long)blockIdx.x * PT_BM;
	const int j0 = blockIdx.y * (NT * 32);
	pt_f32x16 acc[NT];
#pragma unroll
	for (int t = 0; t < NT; ++t)
#pragma unroll
		for (int e = 0; e < 16; ++e)
			acc[t][e] = 0.f;
	const float *xw = xs + (wave * 32 + c) * PT_PITCH + h; // A operand: x[row = lane & 31][k = 2 s + (lane >> 5)]
	const float *aw = as + c * PT_PITCH + h;               // B operand: A[j = lane & 31][k = 2 s + (lane >> 5)]
	float rx[PT_BM * 32 / PT_THREADS], ra[NT * 32 * 32 / PT_THREADS]; // the NEXT chunk, in flight while this one is multiplied
	pt_load<PT_BM, VEC>(rx, a.x, row0, a.n, a.d_in, 0, a.d_in < PT_KC ? a.d_in : PT_KC, tid);
	pt_load<NT * 32, VEC>(ra, a.A, j0, a.d_out, a.d_in, 0, a.d_in < PT_KC ? a.d_in : PT_KC, tid);
	for (int k0 = 0; k0 < a.d_in; k0 += PT_KC) { // (uniform trip counts: every lane reaches every barrier)
		const int kc = a.d_in - k0 < PT_KC ? a.d_in - k0 : PT_KC;
		if (k0 > 0)
			__syncthreads(); // (the previous chunk has been read)
		pt_store<PT_BM, VEC>(xs, rx, tid);
		pt_store<NT * 32, VEC>(as, ra, tid);
		__syncthreads();
		if (k0 + PT_KC < a.d_in) {
			const int kn = a.d_in - k0 - PT_KC < PT_KC ? a.d_in - k0 - PT_KC : PT_KC;
			pt_load<PT_BM, VEC>(rx, a.x, row0, a.n, a.d_in, k0 + PT_KC, kn, tid);
			pt_load<NT * 32, VEC>(ra, a.A, j0, a.d_out, a.d_in, k0 + PT_KC, kn, tid);
		}
		if (kc == PT_KC) {
#pragma unroll
			for (int s = 0; s < PT_KC / 2; ++s) {
				const float av = xw[2 * s];
#pragma unroll
				for (int t = 0; t < NT; ++t)
					acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, aw[t * 32 * PT_PITCH + 2 * s], acc[t], 0, 0, 0);
			}
		} else { // the row's last, partial chunk (an odd kc: the pair's second half is the zero fill)
			const int ns = (kc + 1) >> 1;
			for (int s = 0; s < ns; ++s) {
				const float av = xw[2 * s];
#pragma unroll
				for (int t = 0; t < NT; ++t)
					acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, aw[t * 32 * PT_PITCH + 2 * s], acc[t], 0, 0, 0);
			}
		}
	}
#pragma unroll
	for (int t = 0; t < NT; ++t) {
		const int j = j0 + t * 32 + c;
		if (j >= a.d_out)
			continue;
		const float bias = a.b ? a.b[j] : 0.f;
#pragma unroll
		for (int e = 0; e < 16; ++e) {
			const long long row = row0 + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
			if (row < a.n)
				a.y[(size_t)row * a.d_out + j] = a.b ? __fadd_rn(acc[t][e], bias) : acc[t][e];
		}
	}
}

// one wave per row; every lane walks the same chain over the row (values exchanged by lane broadcast), so nr is the k-ordered chain
__global__ __launch_bounds__(PT_THREADS) void pretransform_l2norm_kernel(const float *x, float *y, long long n, int d) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const long long row = (long long)blockIdx.x * (PT_THREADS / 64) + wave;
	if (row >= n) // (the whole wave; the kernel has no barrier)
		return;
	const float *xr = x + (size_t)row * d;
	float *yr = y + (size_t)row * d;
	float acc = 0.f;
	for (int k0 = 0; k0 < d; k0 += 64) {
		const float v = k0 + lane < d ? xr[k0 + lane] : 0.f;
		const int m = d - k0 < 64 ? d - k0 : 64;
		for (int i = 0; i < m; ++i) {
			const float vi = __shfl(v, i);
			acc = fmaf(vi, vi, acc);
		}
	}
	const bool scale = acc > 0.f; // (a NaN or zero norm: the row is copied)
	// (sqrtf and the division are the correctly rounded ones -- hipcc's default for HIP --, not the __f*_rn intrinsics' native forms)
	const float inv = scale ? 1.0f / sqrtf(acc) : 1.0f;
	for (int k = lane; k < d; k += 64)
		yr[k] = scale ? xr[k] * inv : xr[k];
}

// ---------------------------------------------------------------------------------------------- PCA training (f64, deterministic)
// column sums of row segment s: one thread per column, rows ascending
__global__ void pca_colsum_kernel(const float *x, long long n, int d, long long seglen, double *part /* [S][d] */) {
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= d)
		return;
	const long long r0 = (long long)blockIdx.y * seglen, r1 = r0 + seglen < n ? r0 + seglen : n;
	double s = 0.0;
	for (long long r = r0; r < r1; ++r)
		s += (double)x[(size_t)r * d + j];
	part[(size_t)blockIdx.y * d + j] = s;
}
__global__ void pca_mean_kernel(const double *part, int S, int d, long long n, double *mean) {
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= d)
		return;
	double s = 0.0;
	for (int i = 0; i < S; ++i)
		s += part[(size_t)i * d + j];
	mean[j] = s / (double)n;
}
// partial covariance of row segment blockIdx.z over the 64 x 64 tile (blockIdx.x, blockIdx.y), upper tiles only: thread (ty, tx) owns
// entries (ty + 16 a, tx + 16 b) and adds its products in ascending row order
__global__ __launch_bounds__(256) void pca_cov_kernel(const float *x, long long n, int d, const double *mean, long long seglen,
                                                      double *part /* [S][d][d] */) {
	if (blockIdx.y < blockIdx.x)
		return;
	__shared__ double si[16][64], sj[16][64];
	const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
	const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
	const long long r0 = (long long)blockIdx.z * seglen, r1 = r0 + seglen < n ? r0 + seglen : n;
	double acc[4][4];
#pragma unroll
	for (int p = 0; p < 4; ++p)
#pragma unroll
		for (int q = 0; q < 4; ++q)
			acc[p][q] = 0.0;
	for (long long rb = r0; rb < r1; rb += 16) {
		__syncthreads();
#pragma unroll
		for (int it = 0; it < 4; ++it) {
			const int f = it * 256 + tid, rr = f >> 6, cc = f & 63;
			const long long row = rb + rr;
			const int ci = i0 + cc, cj = j0 + cc;
			si[rr][cc] = row < r1 && ci < d ? (double)x[(size_t)row * d + ci] - mean[ci] : 0.0;
			sj[rr][cc] = row < r1 && cj < d ? (double)x[(size_t)row * d + cj] - mean[cj] : 0.0;
		}
		__syncthreads();
#pragma unroll 4
		for (int rr = 0; rr < 16; ++rr) {
			double ai[4], bj[4];
#pragma unroll
			for (int p = 0; p < 4; ++p)
				ai[p] = si[rr][ty + 16 * p], bj[p] = sj[rr][tx + 16 * p];
#pragma unroll
			for (int p = 0; p < 4; ++p)
#pragma unroll
				for (int q = 0; q < 4; ++q)
					acc[p][q] = fma(ai[p], bj[q], acc[p][q]);
		}
	}
	double *out = part + (size_t)blockIdx.z * d * d;
#pragma unroll
	for (int p = 0; p < 4; ++p)
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const int i = i0 + ty + 16 * p, j = j0 + tx + 16 * q;
			if (i < d && j < d)
				out[(size_t)i * d + j] = acc[p][q];
		}
}
// C[i][j] = (sum over the segments, ascending) / n; an entry of a lower tile is its mirror's (the diagonal tiles hold both halves, equal
// in every bit: the same products in the same order).  V = I
__global__ void pca_cov_reduce_kernel(const double *part, int S, int d, long long n, double *C, double *V) {
	const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= (long long)d * d)
		return;
	const int i = (int)(e / d), j = (int)(e % d);
	const bool upper = (j >> 6) >= (i >> 6);
	const size_t at = upper ? (size_t)i * d + j : (size_t)j * d + i;
	double s = 0.0;
	for (int k = 0; k < S; ++k)
		s += part[(size_t)k * d * d + at];
	C[e] = s / (double)n;
	V[e] = i == j ? 1.0 : 0.0;
}
// one round of the round-robin order: workgroup k orthogonalises columns (p, q) of G = C V, kept as ROWS of G (C is symmetric), and gives V
// the same rotation.  off[k] collects the round's normalised product |<g_p, g_q>| / (|g_p| |g_q|) over a sweep (one writer per launch)
__global__ __launch_bounds__(256) void pca_jacobi_round_kernel(double *G, double *V, int d, int m, int round, double tol, double *off) {
	__shared__ double red[3][256];
	const int k = blockIdx.x, tid = threadIdx.x;
	int p, q;
	if (k == 0) {
		p = m - 1, q = round;
	} else {
		p = (round + k) % (m - 1), q = (round - k + (m - 1)) % (m - 1);
	}
	if (p > q) {
		const int t = p;
		p = q, q = t;
	}
	if (q >= d) // (odd d: the pair with the dummy player; the whole workgroup)
		return;
	double *gp = G + (size_t)p * d, *gq = G + (size_t)q * d;
	double al = 0.0, be = 0.0, ga = 0.0;
	for (int i = tid; i < d; i += 256) {
		const double u = gp[i], v = gq[i];
		al = fma(u, u, al), be = fma(v, v, be), ga = fma(u, v, ga);
	}
	red[0][tid] = al, red[1][tid] = be, red[2][tid] = ga;
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if (tid < s) {
			red[0][tid] += red[0][tid + s];
			red[1][tid] += red[1][tid + s];
			red[2][tid] += red[2][tid + s];
		}
		__syncthreads();
	}
	al = red[0][0], be = red[1][0], ga = red[2][0];
	const double den = sqrt(al) * sqrt(be);
	const double val = den > 0.0 ? fabs(ga) / den : 0.0; // (a zero column is orthogonal to everything)
	if (tid == 0)
		off[k] = fmax(off[k], val);
	if (!(val > tol))
		return;
	const double zeta = (be - al) / (2.0 * ga);
	const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
	const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
	double *vp = V + (size_t)p * d, *vq = V + (size_t)q * d;
	for (int i = tid; i < d; i += 256) {
		const double u = gp[i], v = gq[i];
		gp[i] = cs * u - sn * v;
		gq[i] = sn * u + cs * v;
		const double a = vp[i], b = vq[i];
		vp[i] = cs * a - sn * b;
		vq[i] = sn * a + cs * b;
	}
}

const char *FN_TRAIN = "virtual void faiss::PCAMatrix::train(faiss::idx_t, const float*)";
const char *FILE_VT = "faiss/VectorTransform.cpp";
const char *FN_READ = "faiss::VectorTransform* faiss::read_VectorTransform(faiss::IOReader*)";
const char *FILE_READ = "faiss/impl/index_read.cpp";

// mean [d] f64 and, as rows, the eigenvectors V [d][d] with lambda [d] of the covariance of the device rows x [n][d]
void pca_eigen_device(const float *d_x, int64_t n, int d, std::vector<double> &mean, std::vector<double> &V, std::vector<double> &lambda,
                      hipStream_t st) {
	const int T = (d + 63) / 64;
	const int64_t U = (int64_t)T * (T + 1) / 2;
	int64_t S = std::max<int64_t>(1, (1024 + U - 1) / U);
	S = std::min<int64_t>(S, std::max<int64_t>(1, (n + 63) / 64));
	S = std::min<int64_t>(S, std::max<int64_t>(1, ((int64_t)128 << 20) / ((int64_t)d * d * 8)));
	const int64_t seglen = ((n + S - 1) / S + 15) / 16 * 16;
	S = (n + seglen - 1) / seglen;
	DevBuf part, dmean, dC, dV, doff;
	const size_t dd = (size_t)d * d;
	part.reserve(std::max((size_t)S * dd, (size_t)S * d) * sizeof(double));
	dmean.reserve((size_t)d * sizeof(double));
	dC.reserve(dd * sizeof(double));
	dV.reserve(dd * sizeof(double));
	hipLaunchKernelGGL(pca_colsum_kernel, dim3((d + 255) / 256, (unsigned)S), dim3(256), 0, st, d_x, (long long)n, d, (long long)seglen, (double *)part.p);
	hipLaunchKernelGGL(pca_mean_kernel, dim3((d + 255) / 256), dim3(256), 0, st, (const double *)part.p, (int)S, d, (long long)n, (double *)dmean.p);
	hipLaunchKernelGGL(pca_cov_kernel, dim3(T, T, (unsigned)S), dim3(256), 0, st, d_x, (long long)n, d, (const double *)dmean.p, (long long)seglen,
	                   (double *)part.p);
	hipLaunchKernelGGL(pca_cov_reduce_kernel, dim3((unsigned)((dd + 255) / 256)), dim3(256), 0, st, (const double *)part.p, (int)S, d, (long long)n,
	                   (double *)dC.p, (double *)dV.p);
	MVS_HIP(hipGetLastError());
	const int m = (d + 1) / 2 * 2, npair = m / 2;
	doff.reserve((size_t)npair * sizeof(double));
	std::vector<double> off((size_t)npair);
	bool converged = d < 2;
	for (int sweep = 0; sweep < PT_JACOBI_SWEEPS && !converged; ++sweep) {
		MVS_HIP(hipMemsetAsync(doff.p, 0, (size_t)npair * sizeof(double), st));
		for (int r = 0; r < m - 1; ++r)
			hipLaunchKernelGGL(pca_jacobi_round_kernel, dim3(npair), dim3(256), 0, st, (double *)dC.p, (double *)dV.p, d, m, r, PT_JACOBI_TOL,
			                   (double *)doff.p);
		MVS_HIP(hipGetLastError());
		MVS_HIP(hipMemcpyAsync(off.data(), doff.p, (size_t)npair * sizeof(double), hipMemcpyDeviceToHost, st));
		MVS_HIP(hipStreamSynchronize(st));
		converged = *std::max_element(off.begin(), off.end()) <= PT_JACOBI_TOL;
	}
	if (!converged)
		throw_faiss(FN_TRAIN, FILE_VT, "PCA training: the Jacobi eigensolver has not converged after %d sweeps (d_in = %d)", PT_JACOBI_SWEEPS, d);
	mean.resize((size_t)d);
	V.resize(dd);
	std::vector<double> G(dd);
	MVS_HIP(hipMemcpyAsync(mean.data(), dmean.p, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, st));
	MVS_HIP(hipMemcpyAsync(V.data(), dV.p, dd * sizeof(double), hipMemcpyDeviceToHost, st));
	MVS_HIP(hipMemcpyAsync(G.data(), dC.p, dd * sizeof(double), hipMemcpyDeviceToHost, st));
	MVS_HIP(hipStreamSynchronize(st));
	lambda.assign((size_t)d, 0.0);
	for (int i = 0; i < d; ++i) { // g_i = C v_i, so lambda_i = <v_i, g_i>
		double s = 0.0;
		for (int k = 0; k < d; ++k)
			s = std::fma(V[(size_t)i * d + k], G[(size_t)i * d + k], s);
		lambda[(size_t)i] = s;
	}
}

struct Xform {
	HostTransform h;
	DevBuf dA, db;
	bool on_dev = false;
};

bool valid_vt_type(int t) {
	return t == MVS_VT_LINEAR || t == MVS_VT_PCA || t == MVS_VT_NORM;
}

// what an image or a caller hands over must hold together before anything is built from it
void check_chain(const std::vector<HostTransform> &chain, int d_in, int d_sub) {
	if (chain.empty() || (int)chain.size() > PT_MAX_CHAIN)
		throw_faiss(FN_READ, FILE_READ, "IndexPreTransform with a chain of %zu transforms is not implemented on the MI355X path (1 to %d)", chain.size(),
		            PT_MAX_CHAIN);
	int dc = d_in;
	for (size_t i = 0; i < chain.size(); ++i) {
		const HostTransform &t = chain[i];
		if (!valid_vt_type(t.type))
			throw_faiss(FN_READ, FILE_READ, "IndexPreTransform: unknown transform type %d", t.type);
		if (t.d_in < 1 || t.d_out < 1 || t.d_in > PT_MAX_D || t.d_out > PT_MAX_D)
			throw_faiss(FN_READ, FILE_READ, "IndexPreTransform: transform %zu with d_in = %d, d_out = %d is not implemented on the MI355X path (1 to %d)", i,
			            t.d_in, t.d_out, PT_MAX_D);
		if (t.d_in != dc)
			throw_faiss(FN_READ, FILE_READ, "IndexPreTransform: the chain's dimensions do not join: transform %zu takes d_in = %d where %d arrive", i, t.d_in, dc);
		if (t.type == MVS_VT_NORM) {
			if (t.d_out != t.d_in)
				throw_faiss(FN_READ, FILE_READ, "IndexPreTransform: NormalizationTransform %zu with d_in = %d, d_out = %d", i, t.d_in, t.d_out);
			if (t.norm != 2.0f)
				throw_faiss(FN_READ, FILE_READ, "NormalizationTransform with norm = %g is not implemented on the MI355X path (norm 2 only)", (double)t.norm);
		} else if (t.is_trained) {
			if (t.A.size() != (size_t)t.d_in * t.d_out)
				throw_faiss(FN_READ, FILE_READ, "LinearTransform %zu: A holds %zu values, not d_in * d_out = %d * %d", i, t.A.size(), t.d_in, t.d_out);
			if (t.have_bias && t.b.size() != (size_t)t.d_out)
				throw_faiss(FN_READ, FILE_READ, "LinearTransform %zu: b holds %zu values, not d_out = %d", i, t.b.size(), t.d_out);
		}
		dc = t.d_out;
	}
	if (dc != d_sub)
		throw_faiss(FN_READ, FILE_READ, "IndexPreTransform: the chain's output dimension %d is not the sub-index's d = %d", dc, d_sub);
}

// ---------------------------------------------------------------------------------------------- index
class PretransformIndex : public IndexBase {
public:
	std::vector<Xform> chain;
	IndexBase *sub; // owned
	DevBuf ws[2], ws_in, ws_ids;
	hipStream_t ws_stream = nullptr; // the stream whose work last used the workspaces
	int64_t last_launches = 0, last_ws_bytes = 0;

	PretransformIndex(const std::vector<HostTransform> &hc, IndexBase *sub_) : IndexBase(MVS_KIND_PRETRANSFORM, hc.front().d_in, sub_->metric), sub(sub_) {
		chain.resize(hc.size());
		for (size_t i = 0; i < hc.size(); ++i)
			chain[i].h = hc[i];
		metric_arg = sub->metric_arg;
		ntotal = sub->ntotal;
		refresh_trained();
	}
	~PretransformIndex() override {
		(void)hipSetDevice(device);
		if (stream)
			(void)hipStreamSynchronize(stream);
		delete sub;
	}
	int d_out() const {
		return chain.back().h.d_out;
	}
	bool chain_trained() const {
		for (const Xform &t : chain)
			if (!t.h.is_trained)
				return false;
		return true;
	}
	void adopt_tuning(const Tuning &t) override {
		tune_ = t;
		sub->adopt_tuning(t);
	}
	void refresh_trained() override {
		sub->refresh_trained();
		is_trained = chain_trained() && sub->is_trained;
	}
	void set_label_offset(int64_t off) override {
		label_offset = off;
		sub->set_label_offset(off);
	}
	void require_chain_trained(const char *fn) const {
		if (!chain_trained())
			throw_faiss(fn, "faiss/IndexPreTransform.cpp", "Error: 'is_trained' failed");
	}

	// ------------------------------------------------------------------------------------------ apply
	void upload(Xform &t) {
		if (t.on_dev || t.h.type == MVS_VT_NORM)
			return;
		t.dA.reserve(t.h.A.size() * sizeof(float));
		MVS_HIP(hipMemcpy(t.dA.p, t.h.A.data(), t.h.A.size() * sizeof(float), hipMemcpyHostToDevice));
		if (t.h.have_bias) {
			t.db.reserve(t.h.b.size() * sizeof(float));
			MVS_HIP(hipMemcpy(t.db.p, t.h.b.data(), t.h.b.size() * sizeof(float), hipMemcpyHostToDevice));
		}
		t.on_dev = true;
	}
	void launch_one(Xform &t, int64_t n, const float *d_x, float *d_y, hipStream_t st) {
		const HostTransform &h = t.h;
		if (h.type == MVS_VT_NORM) {
			hipLaunchKernelGGL(pretransform_l2norm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(PT_THREADS), 0, st, d_x, d_y, (long long)n, h.d_in);
		} else {
			upload(t);
			ApplyArgs a;
			a.x = d_x, a.A = (const float *)t.dA.p, a.b = h.have_bias ? (const float *)t.db.p : nullptr, a.y = d_y;
			a.n = n, a.d_in = h.d_in, a.d_out = h.d_out;
			const int NT = h.d_out <= 32 ? 1 : (h.d_out <= 64 ? 2 : (h.d_out <= 128 ? 4 : 8));
			const dim3 grid((unsigned)((n + PT_BM - 1) / PT_BM), (unsigned)((h.d_out + 32 * NT - 1) / (32 * NT)));
			const bool vec = h.d_in % 4 == 0 && ((uintptr_t)d_x & 15) == 0;
#define PT_LAUNCH(NN)                                                                                                                              \
	do {                                                                                                                                           \
		if (vec)                                                                                                                                   \
			hipLaunchKernelGGL((pretransform_apply_kernel<NN, true>), grid, dim3(PT_THREADS), 0, st, a);                                           \
		else                                                                                                                                       \
			hipLaunchKernelGGL((pretransform_apply_kernel<NN, false>), grid, dim3(PT_THREADS), 0, st, a);                                          \
	} while (0)
			if (NT == 1)
				PT_LAUNCH(1);
			else if (NT == 2)
				PT_LAUNCH(2);
			else if (NT == 4)
				PT_LAUNCH(4);
			else
				PT_LAUNCH(8);
#undef PT_LAUNCH
		}
		MVS_HIP(hipGetLastError());
		++last_launches;
	}
	int max_mid_dim(size_t upto) const { // the widest output among transforms [0, upto)
		int m = 0;
		for (size_t i = 0; i < upto; ++i)
			m = std::max(m, chain[i].h.d_out);
		return m;
	}
	// the workspaces change hands between streams only once the previous user has finished with them
	void claim_workspaces(hipStream_t st) {
		if (ws_stream && ws_stream != st)
			MVS_HIP(hipStreamSynchronize(ws_stream));
		ws_stream = st;
	}
	// transforms [0, upto) over d_x [n][d] on `st`; the result lands in `out` if given, else in a workspace.  Returns where it is
	const float *apply_chain(int64_t n, const float *d_x, hipStream_t st, float *out = nullptr, size_t upto = (size_t)-1) {
		upto = std::min(upto, chain.size());
		if (upto == 0 || n <= 0)
			return d_x;
		const size_t nbuf = out ? std::min<size_t>(upto - 1, 2) : std::min<size_t>(upto, 2);
		const size_t bytes = (size_t)n * max_mid_dim(upto) * sizeof(float);
		for (size_t i = 0; i < nbuf; ++i)
			ws[i].reserve(bytes);
		last_ws_bytes += (int64_t)(nbuf * bytes);
		const float *cur = d_x;
		for (size_t i = 0; i < upto; ++i) {
			float *dst = out && i + 1 == upto ? out : (float *)ws[i & 1].p;
			launch_one(chain[i], n, cur, dst, st);
			cur = dst;
		}
		return cur;
	}
	int64_t chunk_rows(bool staged) const {
		const size_t per = sizeof(float) * ((staged ? (size_t)d : 0) + std::min<size_t>(chain.size(), 2) * (size_t)max_mid_dim(chain.size())) +
		                   (staged ? sizeof(int64_t) : 0);
		return std::max<int64_t>(1, (int64_t)(PT_WS_BYTES / per));
	}
	void begin_call(hipStream_t st) {
		use_device();
		last_launches = 0, last_ws_bytes = 0;
		claim_workspaces(st);
	}
	// mvs_index_pretransform_apply / _device: FAISS's apply_chain
	void apply_device(int64_t n, const float *d_x, float *d_out_, hipStream_t st) {
		require_chain_trained("const float* faiss::IndexPreTransform::apply_chain(faiss::idx_t, const float*) const");
		begin_call(st);
		if (n <= 0)
			return;
		apply_chain(n, d_x, st, d_out_);
		MVS_HIP(hipStreamSynchronize(st)); // (the workspaces of the middle steps are free again)
	}
	void apply_host(int64_t n, const float *x, float *out) {
		require_chain_trained("const float* faiss::IndexPreTransform::apply_chain(faiss::idx_t, const float*) const");
		begin_call(stream);
		if (n <= 0)
			return;
		const int dout = d_out();
		const int64_t rows = std::max<int64_t>(1, (int64_t)(PT_WS_BYTES / (sizeof(float) * ((size_t)d + dout + 2 * (size_t)max_mid_dim(chain.size())))));
		const int64_t cap = std::min(n, rows);
		DevBuf outb;
		ws_in.reserve((size_t)cap * d * sizeof(float));
		outb.reserve((size_t)cap * dout * sizeof(float));
		for (int64_t r0 = 0; r0 < n; r0 += rows) {
			const int64_t nc = std::min(rows, n - r0);
			MVS_HIP(hipMemcpyAsync(ws_in.p, x + (size_t)r0 * d, (size_t)nc * d * sizeof(float), hipMemcpyHostToDevice, stream));
			apply_chain(nc, (const float *)ws_in.p, stream, (float *)outb.p);
			MVS_HIP(hipMemcpyAsync(out + (size_t)r0 * dout, outb.p, (size_t)nc * dout * sizeof(float), hipMemcpyDeviceToHost, stream));
			MVS_HIP(hipStreamSynchronize(stream));
		}
		last_ws_bytes = (int64_t)((size_t)cap * sizeof(float) * ((size_t)d + dout + std::min<size_t>(chain.size() - 1, 2) * (size_t)max_mid_dim(chain.size())));
	}

	// ------------------------------------------------------------------------------------------ train
	void train_pca(Xform &t, int64_t n, const float *d_x, hipStream_t st) {
		HostTransform &h = t.h;
		const int di = h.d_in, dout = h.d_out;
		if (n <= 0)
			throw_faiss(FN_TRAIN, FILE_VT, "PCA training needs rows: n = %lld", (long long)n);
		if (n < dout)
			throw_faiss(FN_TRAIN, FILE_VT, "PCA training: n = %lld rows are fewer than d_out = %d", (long long)n, dout);
		std::vector<double> mean, V, lambda;
		pca_eigen_device(d_x, n, di, mean, V, lambda, st);
		std::vector<int> order((size_t)di);
		std::iota(order.begin(), order.end(), 0);
		std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return lambda[(size_t)p] > lambda[(size_t)q]; });
		h.mean.resize((size_t)di), h.eigenvalues.resize((size_t)di), h.PCAMat.resize((size_t)di * di);
		h.A.assign((size_t)dout * di, 0.f), h.b.assign((size_t)dout, 0.f);
		for (int k = 0; k < di; ++k)
			h.mean[(size_t)k] = (float)mean[(size_t)k];
		const bool whiten = h.eigen_power != 0.f;
		for (int i = 0; i < di; ++i) {
			const double *v = &V[(size_t)order[(size_t)i] * di];
			const double lam = lambda[(size_t)order[(size_t)i]];
			int big = 0; // the first component of largest magnitude is made positive (a DEPARTURE: FAISS leaves the sign to LAPACK)
			for (int k = 1; k < di; ++k)
				if (std::fabs(v[k]) > std::fabs(v[big]))
					big = k;
			const double sg = v[big] < 0.0 ? -1.0 : 1.0;
			h.eigenvalues[(size_t)i] = (float)lam;
			for (int k = 0; k < di; ++k)
				h.PCAMat[(size_t)i * di + k] = (float)(sg * v[k]);
			if (i < dout) {
				double scale = 1.0;
				if (whiten) {
					if (!(lam + (double)h.epsilon > 0.0))
						throw_faiss(FN_TRAIN, FILE_VT, "PCAW training: eigenvalue %d is %g: whitening needs positive eigenvalues (epsilon = 0)", i, lam);
					scale = 1.0 / std::sqrt(lam + (double)h.epsilon);
				}
				for (int k = 0; k < di; ++k)
					h.A[(size_t)i * di + k] = (float)(sg * v[k] * scale);
			}
		}
		for (int j = 0; j < dout; ++j) {
			double s = 0.0;
			for (int k = 0; k < di; ++k)
				s += (double)h.A[(size_t)j * di + k] * (double)h.mean[(size_t)k];
			h.b[(size_t)j] = (float)(-s);
		}
		h.have_bias = true;
		h.is_trained = true;
		t.on_dev = false;
	}
	void train(int64_t n, const float *x) override {
		begin_call(stream);
		sub->refresh_trained();
		if (chain_trained() && sub->is_trained) {
			is_trained = true;
			return;
		}
		if (n <= 0) {
			for (const Xform &t : chain)
				if (!t.h.is_trained)
					throw_faiss(FN_TRAIN, FILE_VT, "PCA training needs rows: n = %lld", (long long)n);
			sub->train(n, x);
			refresh_trained();
			return;
		}
		DevBuf cur, nxt; // the whole training set at the current step and at the next
		cur.reserve((size_t)n * d * sizeof(float));
		MVS_HIP(hipMemcpyAsync(cur.p, x, (size_t)n * d * sizeof(float), hipMemcpyHostToDevice, stream));
		const bool need_rows = !sub->is_trained;
		for (size_t i = 0; i < chain.size(); ++i) {
			Xform &t = chain[i];
			if (!t.h.is_trained) // (FAISS's rule: a transform that is trained already is left alone)
				train_pca(t, n, (const float *)cur.p, stream);
			bool later_untrained = false;
			for (size_t j = i + 1; j < chain.size(); ++j)
				later_untrained = later_untrained || !chain[j].h.is_trained;
			if (!need_rows && !later_untrained)
				break;
			nxt.reserve((size_t)n * t.h.d_out * sizeof(float));
			launch_one(t, n, (const float *)cur.p, (float *)nxt.p, stream);
			MVS_HIP(hipStreamSynchronize(stream));
			std::swap(cur.p, nxt.p);
			std::swap(cur.cap, nxt.cap);
		}
		if (need_rows) {
			std::vector<float> y((size_t)n * d_out());
			MVS_HIP(hipMemcpy(y.data(), cur.p, y.size() * sizeof(float), hipMemcpyDeviceToHost));
			cur.release(), nxt.release();
			sub->train(n, y.data());
			use_device();
		}
		refresh_trained();
	}

	// ------------------------------------------------------------------------------------------ add
	void add_host(int64_t n, const float *x, const int64_t *xids) {
		begin_call(stream);
		if (n <= 0)
			return;
		require_chain_trained("virtual void faiss::IndexPreTransform::add(faiss::idx_t, const float*)");
		const int64_t rows = chunk_rows(true), cap = std::min(n, rows);
		ws_in.reserve((size_t)cap * d * sizeof(float));
		if (xids)
			ws_ids.reserve((size_t)cap * sizeof(int64_t));
		for (int64_t r0 = 0; r0 < n; r0 += rows) {
			const int64_t nc = std::min(rows, n - r0);
			MVS_HIP(hipMemcpyAsync(ws_in.p, x + (size_t)r0 * d, (size_t)nc * d * sizeof(float), hipMemcpyHostToDevice, stream));
			if (xids)
				MVS_HIP(hipMemcpyAsync(ws_ids.p, xids + r0, (size_t)nc * sizeof(int64_t), hipMemcpyHostToDevice, stream));
			const float *y = apply_chain(nc, (const float *)ws_in.p, stream);
			if (xids)
				sub->add_with_ids_device(nc, y, (const int64_t *)ws_ids.p, stream);
			else
				sub->add_device(nc, y, stream);
			use_device();
			MVS_HIP(hipStreamSynchronize(stream)); // (the next chunk overwrites the workspaces)
			ntotal = sub->ntotal;
		}
		last_ws_bytes = (int64_t)((size_t)cap * (sizeof(float) * ((size_t)d + std::min<size_t>(chain.size(), 2) * (size_t)max_mid_dim(chain.size())) +
		                                         (xids ? sizeof(int64_t) : 0)));
	}
	void add_dev(int64_t n, const float *d_x, const int64_t *d_ids, hipStream_t st) {
		begin_call(st);
		if (n <= 0)
			return;
		require_chain_trained("virtual void faiss::IndexPreTransform::add(faiss::idx_t, const float*)");
		const int64_t rows = chunk_rows(false);
		for (int64_t r0 = 0; r0 < n; r0 += rows) {
			const int64_t nc = std::min(rows, n - r0);
			const float *y = apply_chain(nc, d_x + (size_t)r0 * d, st);
			if (d_ids)
				sub->add_with_ids_device(nc, y, d_ids + r0, st);
			else
				sub->add_device(nc, y, st);
			use_device();
			MVS_HIP(hipStreamSynchronize(st));
			ntotal = sub->ntotal;
		}
		last_ws_bytes = (int64_t)((size_t)std::min(n, rows) * sizeof(float) * std::min<size_t>(chain.size(), 2) * (size_t)max_mid_dim(chain.size()));
	}
	void add(int64_t n, const float *x) override {
		add_host(n, x, nullptr);
	}
	void add_with_ids(int64_t n, const float *x, const int64_t *xids) override {
		add_host(n, x, xids);
	}
	void add_device(int64_t n, const float *d_x, hipStream_t st) override {
		add_dev(n, d_x, nullptr, st);
	}
	void add_with_ids_device(int64_t n, const float *d_x, const int64_t *d_ids, hipStream_t st) override {
		add_dev(n, d_x, d_ids, st);
	}

	// ------------------------------------------------------------------------------------------ search, range_search, remove_ids
	// (the queries are transformed in one piece: a sub-index may choose its arithmetic by the size of the batch, as FAISS's Flat does)
	void search_mapped(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, const int64_t *d_idmap,
	                   hipStream_t st) override {
		begin_call(st);
		if (k <= 0)
			throw_faiss("virtual void faiss::IndexPreTransform::search(...) const", "faiss/IndexPreTransform.cpp", "Error: 'k > 0' failed");
		require_chain_trained("virtual void faiss::IndexPreTransform::search(...) const");
		if (nq <= 0)
			return;
		const float *y = apply_chain(nq, d_x, st);
		sub->search_mapped(nq, y, k, d_D, d_I, params, d_idmap, st);
		use_device();
		kinfo = sub->kinfo;
	}
	void search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, hipStream_t st) override {
		search_mapped(nq, d_x, k, d_D, d_I, params, nullptr, st);
	}
	void range_search(int64_t nq, const float *x, float radius, const mvs_search_params *params, RangeResult &out) override {
		use_device();
		range_search_mapped(nq, nq > 0 ? stage_queries(nq, x) : nullptr, radius, params, nullptr, out, stream);
	}
	void range_search_mapped(int64_t nq, const float *d_x, float radius, const mvs_search_params *params, const int64_t *d_idmap, RangeResult &out,
	                         hipStream_t st) override {
		begin_call(st);
		require_chain_trained("virtual void faiss::IndexPreTransform::range_search(...) const");
		const float *y = nq > 0 ? apply_chain(nq, d_x, st) : nullptr;
		sub->range_search_mapped(nq, y, radius, params, d_idmap, out, st);
		use_device();
		kinfo = sub->kinfo;
	}
	int64_t remove_ids(const mvs_search_params *sel, const int64_t *d_idmap, RemoveMarks *marks) override {
		const int64_t removed = sub->remove_ids(sel, d_idmap, marks);
		use_device();
		ntotal = sub->ntotal;
		return removed;
	}
	// (recon_source: IndexBase's refusal in FAISS's base-class text -- the reverse transform is out of scope)

	bool set_option(const char *key, int64_t v) override {
		return sub->set_option(key, v);
	}
	bool named_stat(const char *name, int64_t *value) override {
		if (!strcmp(name, "pretransform_apply_launches"))
			*value = last_launches;
		else if (!strcmp(name, "pretransform_workspace_bytes"))
			*value = last_ws_bytes;
		else
			return sub->named_stat(name, value);
		return true;
	}
	bool probe_stats(int64_t *a, int64_t *b, int64_t *c, int64_t *e) override {
		return sub->probe_stats(a, b, c, e);
	}
	bool collect_stats(int64_t *a, int64_t *b, int64_t *c) override {
		return sub->collect_stats(a, b, c);
	}
	size_t device_bytes() const override {
		return sub->device_bytes();
	}
	void set_timing(bool on) override {
		sub->set_timing(on);
	}
	void resolve_timing(int *count, double *total_ms) override {
		sub->resolve_timing(count, total_ms);
		kinfo = sub->kinfo;
	}

	// ------------------------------------------------------------------------------------------ images, placement
	void to_host(HostIndex &out) override {
		refresh_trained();
		out.kind = MVS_KIND_PRETRANSFORM;
		out.d = d;
		out.metric = metric;
		out.metric_arg = metric_arg;
		out.is_trained = is_trained;
		out.chain.clear();
		for (const Xform &t : chain)
			out.chain.push_back(t.h);
		out.sub.reset(new HostIndex);
		sub->to_host(*out.sub);
		out.ntotal = out.sub->ntotal;
	}
	void to_device(int new_device) override {
		if (new_device == device)
			return;
		check_device(new_device);
		sub->to_device(new_device);
		use_device();
		MVS_HIP(hipStreamSynchronize(stream));
		if (ws_stream)
			MVS_HIP(hipStreamSynchronize(ws_stream));
		ws_stream = nullptr;
		for (Xform &t : chain) {
			t.dA.release(), t.db.release();
			t.on_dev = false;
		}
		ws[0].release(), ws[1].release(), ws_in.release(), ws_ids.release();
		move_stream(new_device);
	}
	IndexBase *clone(int on_device) override {
		check_device(on_device);
		HostIndex img;
		to_host(img);
		IndexBase *c = pretransform_from_host(img, on_device);
		c->set_label_offset(label_offset);
		return c;
	}
};

PretransformIndex *as_pt(IndexBase *ix) {
	return ix && ix->kind == MVS_KIND_PRETRANSFORM ? static_cast<PretransformIndex *>(ix) : nullptr;
}
PretransformIndex *need_pt(IndexBase *ix, const char *fn) {
	PretransformIndex *p = as_pt(ix);
	if (!p)
		throw_faiss(fn, __FILE__, "not a PreTransform index");
	return p;
}
Xform &slot_of(PretransformIndex *p, int i, const char *fn) {
	if (i < 0 || i >= (int)p->chain.size())
		throw_faiss(fn, __FILE__, "transform %d of a chain of %zu", i, p->chain.size());
	return p->chain[(size_t)i];
}

bool all_digits(const std::string &s) {
	if (s.empty())
		return false;
	for (char c : s)
		if (c < '0' || c > '9')
			return false;
	return true;
}
// 0: not a transform; 1: PCA<o>; 2: PCAW<o>; 3: L2norm; -1: a FAISS transform this path does not serve
int parse_transform(const std::string &tok, int *o) {
	*o = 0;
	if (tok == "L2norm")
		return 3;
	auto num = [&](size_t at) {
		if (!all_digits(tok.substr(at)) || tok.size() - at > 6)
			return false;
		*o = atoi(tok.c_str() + at);
		return true;
	};
	if (tok.rfind("PCAWR", 0) == 0)
		return num(5) ? -1 : 0;
	if (tok.rfind("PCAW", 0) == 0)
		return num(4) ? 2 : 0;
	if (tok.rfind("PCAR", 0) == 0)
		return num(4) ? -1 : 0;
	if (tok.rfind("PCA", 0) == 0)
		return num(3) ? 1 : 0;
	if (tok.rfind("ITQ", 0) == 0 || tok.rfind("Pad", 0) == 0 || tok.rfind("LDA", 0) == 0)
		return num(3) ? -1 : 0;
	if (tok.rfind("RR", 0) == 0)
		return num(2) ? -1 : 0;
	return 0;
}

} // namespace

// "<t1>,...,<tn>,<sub>" with <t> = PCA<o> | PCAW<o> | L2norm (faiss/index_factory.cpp: the vector transforms come first); nullptr if desc does
// not begin with a transform.  `full` is the whole factory string, for the messages; `sub_factory` makes the sub-index
IndexBase *make_pretransform_index(int d, const std::string &desc, int metric, const std::string &full,
                                   IndexBase *(*sub_factory)(int, const std::string &, int, const std::string &)) {
	const char *fn = "faiss::Index* faiss::index_factory(int, const char*, faiss::MetricType)", *file = "faiss/index_factory.cpp";
	std::vector<HostTransform> chain;
	size_t at = 0;
	int dc = d;
	while (at <= desc.size()) {
		const size_t comma = desc.find(',', at);
		const std::string tok = desc.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
		int o = 0;
		const int what = parse_transform(tok, &o);
		if (what == 0)
			break;
		if (what < 0)
			throw_faiss(fn, file, "This index type is not implemented on the MI355X path yet: %s", full.c_str());
		if (dc > PT_MAX_D)
			throw_faiss(fn, file, "This index type is not implemented on the MI355X path yet: %s (a vector transform of d_in = %d; at most %d)", full.c_str(),
			            dc, PT_MAX_D);
		HostTransform t;
		t.d_in = dc;
		if (what == 3) {
			t.type = MVS_VT_NORM;
			t.d_out = dc;
			t.norm = 2.0f;
			t.is_trained = true;
		} else {
			if (o < 1 || o > dc)
				throw_faiss(fn, file, "%s: the output dimension %d must lie in [1, d_in = %d] (in %s)", tok.c_str(), o, dc, full.c_str());
			t.type = MVS_VT_PCA;
			t.d_out = o;
			t.eigen_power = what == 2 ? -0.5f : 0.f;
			t.have_bias = true;
			t.is_trained = false;
		}
		chain.push_back(t);
		dc = t.d_out;
		if (comma == std::string::npos) { // a chain with no sub-index
			at = desc.size() + 1;
			break;
		}
		at = comma + 1;
	}
	if (chain.empty())
		return nullptr;
	if (at > desc.size() || desc.compare(at, 5, "IDMap") == 0)
		throw_faiss(fn, file, "could not parse index string %s", full.c_str());
	if ((int)chain.size() > PT_MAX_CHAIN)
		throw_faiss(fn, file, "This index type is not implemented on the MI355X path yet: %s (a chain of %zu vector transforms; at most %d)", full.c_str(),
		            chain.size(), PT_MAX_CHAIN);
	IndexBase *sub = sub_factory(dc, desc.substr(at), metric, full);
	try {
		return new PretransformIndex(chain, sub);
	} catch (...) {
		delete sub;
		throw;
	}
}

IndexBase *pretransform_from_host(const HostIndex &h, int device) {
	if (!h.sub)
		throw_faiss(FN_READ, FILE_READ, "IndexPreTransform image without its sub-index");
	if (h.sub->kind == MVS_KIND_IDMAP || h.sub->kind == MVS_KIND_PRETRANSFORM || h.sub->kind == MVS_KIND_REFINE)
		throw_faiss(FN_READ, FILE_READ, "IndexPreTransform over a sub-index of kind %d is not implemented on the MI355X path", h.sub->kind);
	check_chain(h.chain, h.d, h.sub->d);
	CtorDevice scope(device);
	IndexBase *sub = index_from_host(*h.sub, device);
	try {
		return new PretransformIndex(h.chain, sub);
	} catch (...) {
		delete sub;
		throw;
	}
}
IndexBase *pretransform_sub_of(IndexBase *ix) {
	PretransformIndex *p = as_pt(ix);
	return p ? p->sub : nullptr;
}
int pretransform_count(IndexBase *ix) {
	PretransformIndex *p = as_pt(ix);
	return p ? (int)p->chain.size() : -1;
}
void pretransform_info(IndexBase *ix, int i, int *type, int *d_in, int *d_out, int *have_bias, int *is_trained) {
	const char *fn = "mvs_index_pretransform_info";
	const HostTransform &h = slot_of(need_pt(ix, fn), i, fn).h;
	if (type)
		*type = h.type;
	if (d_in)
		*d_in = h.d_in;
	if (d_out)
		*d_out = h.d_out;
	if (have_bias)
		*have_bias = h.type != MVS_VT_NORM && h.have_bias ? 1 : 0;
	if (is_trained)
		*is_trained = h.is_trained ? 1 : 0;
}
void pretransform_get_linear(IndexBase *ix, int i, float *A, float *b) {
	const char *fn = "mvs_index_pretransform_get_linear";
	const HostTransform &h = slot_of(need_pt(ix, fn), i, fn).h;
	if (h.type == MVS_VT_NORM)
		throw_faiss(fn, __FILE__, "transform %d is a normalisation: it has no matrix", i);
	if (!h.is_trained)
		throw_faiss(fn, __FILE__, "transform %d is not trained: it has no matrix yet", i);
	if (A)
		memcpy(A, h.A.data(), h.A.size() * sizeof(float));
	if (b) {
		if (h.have_bias)
			memcpy(b, h.b.data(), h.b.size() * sizeof(float));
		else
			memset(b, 0, (size_t)h.d_out * sizeof(float));
	}
}
void pretransform_set_linear(IndexBase *ix, int i, const float *A, const float *b) {
	const char *fn = "mvs_index_pretransform_set_linear";
	PretransformIndex *p = need_pt(ix, fn);
	Xform &t = slot_of(p, i, fn);
	if (t.h.type == MVS_VT_NORM)
		throw_faiss(fn, __FILE__, "transform %d is a normalisation: it takes no matrix", i);
	if (!A)
		throw_faiss(fn, __FILE__, "null matrix");
	if (p->sub->ntotal != 0)
		throw_faiss(fn, __FILE__, "the index holds %lld rows: a transform can be set only while ntotal == 0", (long long)p->sub->ntotal);
	HostTransform &h = t.h;
	h.type = MVS_VT_LINEAR; // (a PCA slot becomes a plain linear one: its mean and spectrum no longer describe the matrix)
	h.mean.clear(), h.eigenvalues.clear(), h.PCAMat.clear();
	h.A.assign(A, A + (size_t)h.d_in * h.d_out);
	h.have_bias = b != nullptr;
	if (b)
		h.b.assign(b, b + h.d_out);
	else
		h.b.clear();
	h.is_trained = true;
	t.on_dev = false;
	p->refresh_trained();
}
void pretransform_get_pca(IndexBase *ix, int i, float *mean, float *eigenvalues) {
	const char *fn = "mvs_index_pretransform_get_pca";
	const HostTransform &h = slot_of(need_pt(ix, fn), i, fn).h;
	if (h.type != MVS_VT_PCA || !h.is_trained)
		throw_faiss(fn, __FILE__, "transform %d is not a trained PCA", i);
	if (h.mean.size() != (size_t)h.d_in || h.eigenvalues.size() != (size_t)h.d_in)
		throw_faiss(fn, __FILE__, "transform %d holds %zu mean and %zu eigenvalue entries, not d_in = %d", i, h.mean.size(), h.eigenvalues.size(), h.d_in);
	if (mean)
		memcpy(mean, h.mean.data(), h.mean.size() * sizeof(float));
	if (eigenvalues)
		memcpy(eigenvalues, h.eigenvalues.data(), h.eigenvalues.size() * sizeof(float));
}
int pretransform_out_dim(IndexBase *ix) {
	PretransformIndex *p = as_pt(ix);
	return p ? p->d_out() : -1;
}
void pretransform_apply(IndexBase *ix, int64_t n, const float *x, float *out) {
	need_pt(ix, "mvs_index_pretransform_apply")->apply_host(n, x, out);
}
void pretransform_apply_device(IndexBase *ix, int64_t n, const float *d_x, float *d_out, hipStream_t st) {
	need_pt(ix, "mvs_index_pretransform_apply_device")->apply_device(n, d_x, d_out, st);
}

} // namespace mvs
