// csrc/ivfpqfs.hip -- faiss::IndexIVFPQFastScan: inverted lists of 4-bit product-quantised RESIDUALS, scanned on the int8 matrix pipe.
// MVS_KIND_IVFPQFS, reached through mvs_index_ivfpqfs_new (the factory keeps refusing "IVF<n>,PQ<M>x4fs").
//
// Contract (include/mi355_faiss.h "inverted lists of 4-bit product-quantised residuals"):
//   train   IVFPQ's rule with 16 centroids: coarse centroids as IVF<n>,Flat; codebook m = what IVF16,Flat (L2) learns from the residuals' columns
//   add     list = the quantiser's k = 1 label; code = PQFS's encoding rule on x - c; FAISS's packing, M / 2 bytes a row
//   search  per (query x, probed list with centroid c): T[m][j] = IVFPQ's chain over 16 entries (L2: v = x - c; inner product: v = x,
//           base = the chain <x, c>); lo_m, hi_m, span, a = 255 / span, tq as PQFS; b = ((lo_0 + lo_1) + ...) / (((base + lo_0) + lo_1) + ...);
//           s = sum_m tq[m][code_m]; dis = b + (float)s / a (a == 0: b); IVFPQ's PURE order and PQ's admission rule
//
// The host driver is CodedListsIndex (csrc/coded_lists.hip): it hands the scan the (query, probe rank) pairs of a unit grouped by list.
// Grouped by list is the shape an MFMA scan needs: the pairs of one list are the A tiles, the rows of that list the B tiles.
//
// Kernels
//   ivfpqfs_residual_encode_kernel  one lane per (row, code byte): the residual's two sub-vectors against 16 entries each, two nibbles out
//   ivfpqfs_tables_kernel           per chunk, before the units: a workgroup walks (query, rank) pairs with the codebooks in LDS; per pair
//                                   v, the M x 16 chains, lo / hi / span, (a, b), a validity flag and the bytes tq - 128 as [pair][4 S][16]:
//                                   the 16 bytes of one (pair, m) are one lane's A operand
//   ivfpqfs_scan_kernel<T, SMAX>    the hot path, list- and pair-stationary: a workgroup = (<= Q = 16 T pairs of one list, one segment of R
//                                   positions); every wave gathers the A fragments of the group's pair tiles into registers, the four waves
//                                   take different 16-row tiles.  A lane loads its row's nibbles once per tile and expands them into one-hot
//                                   B operands; a group of p pairs issues MFMAs for ceil(p / 16) tiles only.  The query's bound is moved to
//                                   the integer side once per workgroup; only a hit forms b + s / a, re-tests it exactly, applies the
//                                   selector and writes (order key, ordinal) to the query's bucket (CodedListsIndex's overflow protocol)
#include "coded_lists.h"
#include "pq_kernels.h"
#include "pqfs_kernels.h"

#include <algorithm>
#include <climits>
#include <cstring>

namespace mvs {

namespace {

constexpr int IVFPQFS_ROWS_PER_WG = PQ_ROWS_PER_WG; // positions of a list one scan workgroup walks = bucket entries
constexpr int IVFPQFS_SCAN_THREADS = 256;           // four waves, one per SIMD
constexpr size_t IVFPQFS_CB_LDS_MAX = (size_t)128 << 10; // the codebooks go to the table kernel's LDS up to here (d <= 2048)
constexpr int IVFPQFS_S_TOP = 255 * PQFS_MAX_M;     // no score is above it

// ---------------------------------------------------------------------------------------------- encode
// rows x [n][d] of lists label -> code bytes of rows [row0, row0 + n): byte i holds sub-quantiser 2 i (low nibble) and 2 i + 1
__global__ __launch_bounds__(256) void ivfpqfs_residual_encode_kernel(const float *__restrict__ x, long long n, int d, int M, int dsub,
                                                                      const long long *__restrict__ label, const float *__restrict__ cent, long long nlist,
                                                                      const float *__restrict__ cb, unsigned char *__restrict__ codes, int pitch, long long row0) {
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	const int hb = M / 2;
	const long long r = i / hb;
	if (r >= n)
		return;
	const int byte = (int)(i - r * hb);
	const long long l = label[r];
	const float *c = l >= 0 && l < nlist ? cent + l * d : nullptr; // (a row without a list is stored nowhere: its code is never read)
	unsigned out = 0;
	for (int h = 0; h < 2; ++h) {
		const int m = 2 * byte + h;
		const float *xv = x + r * d + (long long)m * dsub;
		float best = 0.f;
		unsigned bj = 0;
		for (int j = 0; j < PQFS_KSUB; ++j) {
			const float *cj = cb + ((size_t)m * PQFS_KSUB + j) * dsub;
			float acc = 0.f;
			for (int k = 0; k < dsub; ++k) {
				const float v = c ? xv[k] - c[m * dsub + k] : xv[k]; // the residual: one f32 subtraction per component
				const float t = v - cj[k];
				acc = fmaf(t, t, acc);
			}
			if (j == 0 || acc < best) {
				best = acc;
				bj = (unsigned)j;
			}
		}
		out |= bj << (4 * h);
	}
	codes[(row0 + r) * pitch + byte] = (unsigned char)out;
}

// x - centroid[label] (training: the residuals go back to the host)
__global__ __launch_bounds__(256) void ivfpqfs_residual_kernel(const float *__restrict__ x, long long n, int d, const long long *__restrict__ label,
                                                               const float *__restrict__ cent, long long nlist, float *__restrict__ out) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n * d)
		return;
	const long long r = i / d;
	const long long l = label[r];
	out[i] = l >= 0 && l < nlist ? x[i] - cent[l * d + (i - r * d)] : x[i];
}

// ---------------------------------------------------------------------------------------------- tables
struct IvfpqfsTables {
	const float *xq;      // the chunk's queries [nqc][d]
	const long long *cI;  // their probed lists [nqc][np]
	const float *cent;    // [nlist][d]
	const float *cb;      // [M][16][dsub]
	long long npairs;     // nqc np
	int np, nlist, d, M, dsub, S, is_l2, cb_in_lds;
	pqfs_i32x4 *tabs;     // [pair][4 S]: the 16 bytes tq - 128 of (pair, m); m >= M: zero
	float2 *ab;           // [pair] (a, b)
	int *flag;            // [pair] 1: the pair contributes no row (no list, a non-finite table entry or base)
};
// LDS: T [128][16] | lo [128] | hi [128] | v [d] | codebooks [16 d] (cb_in_lds)
__global__ __launch_bounds__(256) void ivfpqfs_tables_kernel(const IvfpqfsTables a) {
	extern __shared__ __attribute__((aligned(16))) float ivfpqfs_tab_lds[];
	__shared__ float s_a, s_base;
	__shared__ int s_bad;
	float *T = ivfpqfs_tab_lds, *lo = T + PQFS_MAX_M * PQFS_KSUB, *hi = lo + PQFS_MAX_M, *v = hi + PQFS_MAX_M, *cbs = v + a.d;
	const int tid = threadIdx.x, M = a.M, d = a.d, dsub = a.dsub;
	if (a.cb_in_lds)
		for (int i = tid; i < PQFS_KSUB * d; i += 256)
			cbs[i] = a.cb[i];
	const float *cb = a.cb_in_lds ? cbs : a.cb;
	for (long long pair = blockIdx.x; pair < a.npairs; pair += gridDim.x) {
		const long long q = pair / a.np, l = a.cI[pair];
		if (l < 0 || l >= a.nlist) { // (uniform over the workgroup) a -1 probe: no unit ever holds the pair
			if (tid == 0)
				a.flag[pair] = 1;
			continue;
		}
		__syncthreads(); // (the previous pair's T, lo, v are read no more)
		const float *x = a.xq + q * d, *c = a.cent + l * d;
		for (int k = tid; k < d; k += 256)
			v[k] = a.is_l2 ? x[k] - c[k] : x[k];
		if (tid == 0)
			s_bad = 0;
		__syncthreads();
		for (int e = tid; e < M * PQFS_KSUB; e += 256) {
			const float t = pqfs_chain(v + (e >> 4) * dsub, cb + (size_t)e * dsub, dsub, a.is_l2);
			T[e] = t;
			if (!(fabsf(t) <= FLT_MAX)) // NaN or inf
				s_bad = 1;
		}
		if (tid == 255) { // base = the ip chain <x, c>, k ascending
			float acc = 0.f;
			if (!a.is_l2)
				for (int k = 0; k < d; ++k)
					acc = fmaf(x[k], c[k], acc);
			s_base = acc;
			if (!(fabsf(acc) <= FLT_MAX))
				s_bad = 1;
		}
		__syncthreads();
		if (tid < M) {
			float l0 = T[tid * PQFS_KSUB], h0 = l0;
			for (int j = 1; j < PQFS_KSUB; ++j) {
				l0 = fminf(l0, T[tid * PQFS_KSUB + j]);
				h0 = fmaxf(h0, T[tid * PQFS_KSUB + j]);
			}
			lo[tid] = l0, hi[tid] = h0;
		}
		__syncthreads();
		if (tid == 0) {
			float span = 0.f, b = a.is_l2 ? lo[0] : __fadd_rn(s_base, lo[0]);
			for (int m = 0; m < M; ++m) {
				span = fmaxf(span, __fsub_rn(hi[m], lo[m]));
				if (m > 0)
					b = __fadd_rn(b, lo[m]);
			}
			const float qa = s_bad || span == 0.f ? 0.f : __fdiv_rn(255.f, span);
			a.ab[pair] = make_float2(qa, b);
			a.flag[pair] = s_bad;
			s_a = qa;
		}
		__syncthreads();
		const float qa = s_a;
		for (int m = tid; m < 4 * a.S; m += 256)
			a.tabs[pair * (4 * a.S) + m] = m < M ? pqfs_quantise16(T + m * PQFS_KSUB, lo[m], qa) : pqfs_i32x4 {0, 0, 0, 0};
	}
}

// ---------------------------------------------------------------------------------------------- scan
struct IvfpqfsScan : CodedScan { // par: the codebooks (not read by the scan); codes: rows of pitch = 16 ceil(M / 32) bytes, FAISS's packing
	const pqfs_i32x4 *tabs;
	const float2 *ab;
	const int *flag;
	int M, S, is_l2;
};

// A pair's bound on the accumulator's side.  u = dis (L2) / -dis (inner product) must be below th (pq_bound_value); with sgn = +1 / -1 that
// is sgn s < (th - sgn b) a.  The f32 roundings of b + (float)s / a move a value by less than `slack` score units, so every s the exact
// test can admit passes sgn acc < bound; INT_MIN admits nothing, INT_MAX everything (the exact test follows a hit)
__device__ __forceinline__ int ivfpqfs_bound(float th, float a, float b, int descending, int bias) {
	if (!(th == th))
		return INT_MIN; // (thr == 0: no key is below it)
	if (a == 0.f)
		return INT_MAX; // every score prints b
	const double sgn = descending ? -1.0 : 1.0;
	const double x = ((double)th - sgn * (double)b) * (double)a;
	const double slack = 2.0 + ((fabs((double)th) + fabs((double)b)) * (double)a + (double)IVFPQFS_S_TOP) * (1.0 / 4194304.0);
	const double top = x + slack;
	if (!(top == top) || top <= -(double)(IVFPQFS_S_TOP + 1))
		return INT_MIN;
	if (top >= (double)(IVFPQFS_S_TOP + 1))
		return INT_MAX;
	return (int)ceil(top) - (descending ? -bias : bias);
}

// the rows of positions [s0, s1) of the list at lb against NT pair tiles whose A fragments are af
template <int T, int SMAX, int NT>
__device__ __forceinline__ void ivfpqfs_walk(const IvfpqfsScan &a, const pqfs_i32x4 (&af)[T][SMAX], const int (&bnd)[T][4], long long lb, long long s0,
                                             long long s1, const int *s_q, const unsigned *s_ord, const float *s_a, const float *s_b, const float *s_th) {
	constexpr int CH = SMAX > 8 ? SMAX / 8 : 1; // 16-byte words of a row at most
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int descending = a.is_l2 ? 0 : 1, bias = 128 * a.M, words = a.pitch >> 4, S = a.S;
	const unsigned smask = pq_sign_mask(descending);
	const int ntile = (int)((s1 - s0 + 15) >> 4);
	const uint4 *rows = reinterpret_cast<const uint4 *>(a.codes);
	unsigned cur[CH][4], nxt[CH][4];
	auto load = [&](int tl, unsigned (&w)[CH][4]) {
		const long long pos = s0 + 16ll * tl + (lane & 15);
#pragma unroll
		for (int c = 0; c < CH; ++c) {
			const uint4 u = tl < ntile && pos < s1 && c < words ? rows[(lb + pos) * words + c] : make_uint4(0u, 0u, 0u, 0u);
			w[c][0] = u.x, w[c][1] = u.y, w[c][2] = u.z, w[c][3] = u.w;
		}
	};
	load(wave, cur);
	for (int tl = wave; tl < ntile; tl += 4) {
		load(tl + 4, nxt);
		pqfs_i32x4 acc[NT];
#pragma unroll
		for (int t = 0; t < NT; ++t)
			acc[t] = pqfs_i32x4 {0, 0, 0, 0};
#pragma unroll
		for (int st = 0; st < SMAX; ++st) {
			if (st < S) { // (wave-uniform) sub-quantiser 4 st + g, g = lane >> 4: nibble 4 (st & 1) + g of dword st / 2 of the row
				const pqfs_i32x4 b = pqfs_one_hot((cur[st >> 3][(st >> 1) & 3] >> (16 * (st & 1) + 4 * (lane >> 4))) & 15u);
#pragma unroll
				for (int t = 0; t < NT; ++t)
					acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[t][st], b, acc[t], 0, 0, 0);
			}
		}
		// acc[t][i]: pair 4 (lane >> 4) + i of tile t against row lane & 15 of the row tile
		bool any = false;
#pragma unroll
		for (int t = 0; t < NT; ++t)
#pragma unroll
			for (int i = 0; i < 4; ++i)
				any |= (descending ? -acc[t][i] : acc[t][i]) < bnd[t][i];
		const long long pos = s0 + 16ll * tl + (lane & 15);
		if (any && pos < s1) {
			bool member = true;
			if (a.sel.kind != MVS_SEL_NONE) {
				const long long id = a.lids[lb + pos];
				member = pq_sel_member(a.sel, a.idmap ? a.idmap[id] : id);
			}
			if (member) {
#pragma unroll
				for (int t = 0; t < NT; ++t)
#pragma unroll
					for (int i = 0; i < 4; ++i)
						if ((descending ? -acc[t][i] : acc[t][i]) < bnd[t][i]) {
							const int slot = t * 16 + 4 * (lane >> 4) + i;
							const float s = (float)(acc[t][i] + bias), qa = s_a[slot];
							const float dis = qa == 0.f ? s_b[slot] : __fadd_rn(s_b[slot], __fdiv_rn(s, qa));
							if (pq_beats(dis, s_th[slot], smask)) {
								const int q = s_q[slot];
								const unsigned at = atomicAdd(&a.cnt[q], 1u);
								if (at < (unsigned)IVFPQFS_ROWS_PER_WG)
									a.bucket[(size_t)q * IVFPQFS_ROWS_PER_WG + at] =
									    ((unsigned long long)pq_key(dis, descending) << 32) | (unsigned long long)(s_ord[slot] + (unsigned)pos);
								else
									*a.overflow = 1;
							}
						}
			}
		}
#pragma unroll
		for (int c = 0; c < CH; ++c)
#pragma unroll
			for (int w = 0; w < 4; ++w)
				cur[c][w] = nxt[c][w];
	}
}

// workgroup blockIdx.x = one pair group (<= Q = 16 T pairs of one list), blockIdx.y = the segment of R positions of the window.  SMAX: the
// steps the instance unrolls, a power of two >= S = ceil(M / 4).  T SMAX <= 64: 256 of a lane's registers hold A fragments
template <int T, int SMAX>
__global__ __launch_bounds__(IVFPQFS_SCAN_THREADS) void ivfpqfs_scan_kernel(const IvfpqfsScan a) {
	constexpr int Q = 16 * T;
	__shared__ int s_q[Q], s_pi[Q], s_bnd[Q];
	__shared__ unsigned s_ord[Q];
	__shared__ float s_a[Q], s_b[Q], s_th[Q];
	const int tid = threadIdx.x, lane = tid & 63, g = blockIdx.x;
	if (g >= a.goff[a.nlist])
		return;
	int lo = 0, hi = a.nlist; // the list with goff[l] <= g < goff[l + 1]
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (a.goff[mid] <= g)
			lo = mid;
		else
			hi = mid;
	}
	const int l = lo;
	const long long lb = a.list_off[l], ls = a.list_off[l + 1] - lb;
	const long long w1 = ls < a.p1 ? ls : a.p1;
	const long long s0 = a.p0 + (long long)blockIdx.y * IVFPQFS_ROWS_PER_WG;
	if (s0 >= w1)
		return; // (uniform over the workgroup: no barrier has been reached)
	const long long s1 = s0 + IVFPQFS_ROWS_PER_WG < w1 ? s0 + IVFPQFS_ROWS_PER_WG : w1;
	const int pj = a.poff[l] + (g - a.goff[l]) * Q;
	const int npg = a.poff[l + 1] - pj < Q ? a.poff[l + 1] - pj : Q; // pairs of this group, >= 1
	const int descending = a.is_l2 ? 0 : 1;
	if (tid < Q) {
		int q = 0, pi = 0, bnd = INT_MIN; // a slot without a pair, and an invalid pair, never hit
		unsigned ord = 0;
		float qa = 0.f, qb = 0.f, th = 0.f;
		if (tid < npg) {
			const int2 p = a.pairs[pj + tid];
			q = p.x, pi = p.x * a.np + p.y;
			ord = a.pref[(size_t)p.x * (a.np + 1) + p.y];
			const float2 ab = a.ab[pi];
			qa = ab.x, qb = ab.y;
			th = pq_bound_value(a.thr[q], descending);
			if (!a.flag[pi])
				bnd = ivfpqfs_bound(th, qa, qb, descending, 128 * a.M);
		}
		s_q[tid] = q, s_pi[tid] = pi, s_bnd[tid] = bnd, s_ord[tid] = ord, s_a[tid] = qa, s_b[tid] = qb, s_th[tid] = th;
	}
	__syncthreads();
	const int nt = (npg + 15) >> 4; // pair tiles that exist
	// A fragments: lane -> pair lane & 15 of the tile, sub-quantiser 4 st + (lane >> 4): the 16 bytes of (pair, m)
	pqfs_i32x4 af[T][SMAX];
	int bnd[T][4];
#pragma unroll
	for (int t = 0; t < T; ++t) {
		const int slot = t * 16 + (lane & 15);
		const pqfs_i32x4 *src = a.tabs + (size_t)s_pi[slot] * (4 * a.S) + (lane >> 4);
#pragma unroll
		for (int st = 0; st < SMAX; ++st)
			af[t][st] = slot < npg && st < a.S ? src[4 * st] : pqfs_i32x4 {0, 0, 0, 0};
#pragma unroll
		for (int i = 0; i < 4; ++i)
			bnd[t][i] = s_bnd[t * 16 + 4 * (lane >> 4) + i];
	}
#define IVFPQFS_WALK(NT)                                                                                                                            \
	case NT:                                                                                                                                        \
		if constexpr (NT <= T)                                                                                                                      \
			ivfpqfs_walk<T, SMAX, NT>(a, af, bnd, lb, s0, s1, s_q, s_ord, s_a, s_b, s_th);                                                          \
		break
	switch (nt) { // (wave-uniform) a group of p pairs issues MFMAs for ceil(p / 16) tiles only
		IVFPQFS_WALK(1);
		IVFPQFS_WALK(2);
		IVFPQFS_WALK(3);
		IVFPQFS_WALK(4);
		IVFPQFS_WALK(5);
		IVFPQFS_WALK(6);
		IVFPQFS_WALK(7);
		IVFPQFS_WALK(8);
	}
#undef IVFPQFS_WALK
}

// ---------------------------------------------------------------------------------------------- index
[[noreturn]] void ivfpqfs_refuse(const char *fn, const char *file, const char *what) {
	throw_faiss(fn, file, "This index type is not implemented on the MI355X path yet: %s over IndexIVFPQFastScan", what);
}

class IVFPQFSIndex : public CodedListsIndex {
public:
	const int M, dsub, S; // S = ceil(M / 4) MFMA steps
	DevBuf ws_tabs, ws_ab, ws_flag; // the chunk's tables, (a, b) and validity flags, [nqc np] pairs

	IVFPQFSIndex(int d_, int64_t nlist_, int M_, int metric_)
	    : CodedListsIndex(MVS_KIND_IVFPQFS, d_, metric_, nlist_, M_ / 2, (size_t)M_ * PQFS_KSUB * (d_ / M_), false,
	                      {"mvs::IVFPQFSIndex", __FILE__, "IVFPQFastScan", "IVFPQFastScan", "virtual void faiss::IndexIVFFastScan::add_with_ids(...)",
	                       "faiss/IndexIVFFastScan.cpp", "ivfpqfs", nullptr}),
	      M(M_), dsub(d_ / M_), S((M_ + 3) / 4) {
	}

	// ------------------------------------------------------------------------------------------ train
	void check_empty_for_training() const override {
		if (ntotal > 0)
			throw_faiss("mvs::IVFPQFSIndex::train", __FILE__, "the index already holds %lld rows encoded with its centroids and codebooks: "
			            "training again is only possible while it is empty", (long long)ntotal);
	}
	void set_codebooks(const float *c) {
		use_device();
		check_empty_for_training();
		ensure_par();
		MVS_HIP(hipMemcpyAsync(d_par(), c, par_floats * sizeof(float), hipMemcpyHostToDevice, stream));
		MVS_HIP(hipStreamSynchronize(stream));
		have_par = true;
		++params_epoch;
		update_trained();
	}
	void get_codebooks(float *out) {
		use_device();
		if (!d_par())
			throw_faiss("mvs::IVFPQFSIndex::get_centroids", __FILE__, "the index has no codebooks yet");
		MVS_HIP(hipStreamSynchronize(stream));
		MVS_HIP(hipMemcpy(out, d_par(), par_floats * sizeof(float), hipMemcpyDeviceToHost));
	}
	void train(int64_t n, const float *x) override { // csrc/ivfpq.hip's three steps with 16 centroids a codebook
		use_device();
		check_empty_for_training();
		n = std::max<int64_t>(n, 0);
		CtorDevice scope(device);
		train_coarse(n, x);
		std::vector<float> res((size_t)n * d);
		const int64_t bs = 65536;
		ws_add.reserve((size_t)std::min(bs, n) * d * sizeof(float));
		ws_kind.reserve((size_t)std::min(bs, n) * d * sizeof(float));
		ws_lab.reserve((size_t)std::min(bs, n) * (sizeof(float) + sizeof(int64_t)));
		for (int64_t i0 = 0; i0 < n; i0 += bs) {
			const int64_t nb = std::min(bs, n - i0);
			MVS_HIP(hipMemcpyAsync(ws_add.p, x + i0 * d, (size_t)nb * d * sizeof(float), hipMemcpyHostToDevice, stream));
			int64_t *d_lab = (int64_t *)ws_lab.p;
			assign_device(nb, (const float *)ws_add.p, (float *)(d_lab + nb), d_lab);
			const long long tot = nb * d;
			hipLaunchKernelGGL(ivfpqfs_residual_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, (const float *)ws_add.p, (long long)nb, d,
			                   (const long long *)d_lab, centroids_dev(), (long long)nlist, (float *)ws_kind.p);
			MVS_HIP(hipGetLastError());
			MVS_HIP(hipMemcpyAsync(&res[(size_t)i0 * d], ws_kind.p, (size_t)nb * d * sizeof(float), hipMemcpyDeviceToHost, stream));
			MVS_HIP(hipStreamSynchronize(stream));
		}
		std::vector<float> cent(par_floats), cols((size_t)n * dsub);
		for (int m = 0; m < M; ++m) {
			for (int64_t i = 0; i < n; ++i)
				memcpy(&cols[(size_t)i * dsub], &res[(size_t)i * d + (size_t)m * dsub], (size_t)dsub * sizeof(float));
			FlatIndex assigner(dsub, METRIC_L2);
			assigner.adopt_tuning(tune_);
			kmeans_train({PQFS_KSUB, 10, false}, n, cols.data(), assigner);
			assigner.copy_rows_to_host(&cent[(size_t)m * PQFS_KSUB * dsub]);
		}
		set_codebooks(cent.data());
	}

	// ------------------------------------------------------------------------------------------ add, search: what CodedListsIndex asks for
	void encode_block(int64_t nb, const float *d_x, const int64_t *d_lab, int64_t first_row) override {
		const long long tot = nb * (M / 2);
		hipLaunchKernelGGL(ivfpqfs_residual_encode_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, d_x, (long long)nb, d, M, dsub,
		                   (const long long *)d_lab, centroids_dev(), (long long)nlist, (const float *)d_par(), store.codes(), store.pitch, (long long)first_row);
	}
	// the instance: SMAX the power of two that holds S steps, T SMAX <= 64, T <= 8
	int smax() const {
		int s = 2;
		while (s < S)
			s <<= 1;
		return s;
	}
	int pair_block() const override {
		return 16 * std::min(8, 64 / smax());
	}
	size_t pair_bytes() const { // table bytes of one (query, rank) pair
		return (size_t)4 * S * sizeof(pqfs_i32x4);
	}
	int64_t chunk_query_cap(int64_t np) const override { // the chunk's tables stay within what the buckets are allowed
		return (int64_t)(PQ_BUCKET_SCRATCH / (pair_bytes() * (size_t)np));
	}
	int prepare_chunk(int64_t nqc, const float *d_xq, const int64_t *d_cI, int np) override {
		const int64_t npairs = nqc * np;
		ws_tabs.reserve((size_t)npairs * pair_bytes());
		ws_ab.reserve((size_t)npairs * sizeof(float2));
		ws_flag.reserve((size_t)npairs * sizeof(int));
		IvfpqfsTables t;
		t.xq = d_xq, t.cI = (const long long *)d_cI, t.cent = centroids_dev(), t.cb = d_par();
		t.npairs = npairs, t.np = np, t.nlist = (int)nlist, t.d = d, t.M = M, t.dsub = dsub, t.S = S, t.is_l2 = metric == METRIC_L2 ? 1 : 0;
		const size_t cb_bytes = (size_t)PQFS_KSUB * d * sizeof(float);
		t.cb_in_lds = cb_bytes <= IVFPQFS_CB_LDS_MAX ? 1 : 0;
		t.tabs = (pqfs_i32x4 *)ws_tabs.p, t.ab = (float2 *)ws_ab.p, t.flag = (int *)ws_flag.p;
		const size_t lds = ((size_t)PQFS_MAX_M * (PQFS_KSUB + 2) + d) * sizeof(float) + (t.cb_in_lds ? cb_bytes : 0);
		ensure_dynamic_lds((const void *)ivfpqfs_tables_kernel, lds);
		// every workgroup loads the codebooks once and walks pairs: a few workgroups per compute unit
		hipLaunchKernelGGL(ivfpqfs_tables_kernel, dim3((unsigned)std::min<int64_t>(npairs, 2048)), dim3(256), lds, stream, t);
		MVS_HIP(hipGetLastError());
		return 1;
	}
	void launch_scan_kernel(const CodedScan &c, dim3 grid, int64_t nqc, double rows) override {
		IvfpqfsScan a;
		static_cast<CodedScan &>(a) = c;
		a.tabs = (const pqfs_i32x4 *)ws_tabs.p, a.ab = (const float2 *)ws_ab.p, a.flag = (const int *)ws_flag.p;
		a.M = M, a.S = S, a.is_l2 = metric == METRIC_L2 ? 1 : 0;
#define IVFPQFS_LAUNCH_SCAN(TT, SS) hipLaunchKernelGGL((ivfpqfs_scan_kernel<TT, SS>), grid, dim3(IVFPQFS_SCAN_THREADS), 0, stream, a)
		switch (smax()) {
		case 2:
			IVFPQFS_LAUNCH_SCAN(8, 2);
			break;
		case 4:
			IVFPQFS_LAUNCH_SCAN(8, 4);
			break;
		case 8:
			IVFPQFS_LAUNCH_SCAN(8, 8);
			break;
		case 16:
			IVFPQFS_LAUNCH_SCAN(4, 16);
			break;
		default:
			IVFPQFS_LAUNCH_SCAN(2, 32);
			break;
		}
#undef IVFPQFS_LAUNCH_SCAN
		// 2 K ops per (pair, row) of the GEMM, K = 16 slots a sub-quantiser over 4 S of them; bytes: every pair group reads its rows' codes
		set_kinfo("ivfpqfs_scan_kernel", 2.0 * 16.0 * 4.0 * S * (double)nqc * rows, (double)nqc * rows * store.pitch / pair_block(), (int)(grid.x * grid.y),
		          IVFPQFS_SCAN_THREADS, 0, (int)grid.y);
	}
	void release_kind_device() override {
		ws_tabs.release();
		ws_ab.release();
		ws_flag.release();
	}

	// ------------------------------------------------------------------------------------------ what the kind does not serve
	void range_search(int64_t, const float *, float, const mvs_search_params *, RangeResult &) override {
		ivfpqfs_refuse("virtual void faiss::Index::range_search(...) const", "faiss/Index.cpp", "range_search");
	}
	void range_search_mapped(int64_t, const float *, float, const mvs_search_params *, const int64_t *, RangeResult &, hipStream_t) override {
		ivfpqfs_refuse("virtual void faiss::Index::range_search(...) const", "faiss/Index.cpp", "range_search");
	}

	// ------------------------------------------------------------------------------------------ images (this path's own: clone, to_gpu)
	void check_image(const HostIndex &h) const override {
		if ((int64_t)h.list_ids.size() != nlist || (int64_t)h.list_bytes.size() != nlist || h.pq_centroids.size() != par_floats)
			throw_faiss("mvs::IVFPQFSIndex::load_image", __FILE__, "IVFPQFastScan image: inverted lists or codebooks do not match nlist = %lld, d = %d, M = %d",
			            (long long)nlist, d, M);
	}
	void params_to_host(HostIndex &out) override {
		out.pq_M = M;
		out.pq_centroids.assign(par_floats, 0.f);
		if (have_par)
			get_codebooks(out.pq_centroids.data());
	}
	void params_from_host(const HostIndex &h) override {
		bool any = false;
		for (float v : h.pq_centroids)
			any = any || v != 0.f;
		if (h.is_trained || any)
			set_codebooks(h.pq_centroids.data());
	}
};

IVFPQFSIndex *as_ivfpqfs(IndexBase *ix) {
	return ix && ix->kind == MVS_KIND_IVFPQFS ? static_cast<IVFPQFSIndex *>(ix) : nullptr;
}

bool ivfpqfs_geometry_ok(int d, int64_t nlist, int M) {
	return nlist > 0 && M >= 2 && M % 2 == 0 && M <= PQFS_MAX_M && d > 0;
}

} // namespace

// faiss::IndexIVFPQFastScan(quantizer, d, nlist, M, nbits, metric) with an own Flat quantiser
IndexBase *make_ivfpqfs_index(int d, int64_t nlist, int M, int nbits, int metric) {
	const char *fn = "faiss::IndexIVFPQFastScan::IndexIVFPQFastScan(faiss::Index*, size_t, size_t, size_t, size_t, faiss::MetricType, int)";
	const char *file = "faiss/IndexIVFPQFastScan.cpp";
	if (nbits != 4)
		throw_faiss(fn, file, "This index type is not implemented on the MI355X path yet: IndexIVFPQFastScan with nbits = %d (4 bits per code only)", nbits);
	if (!ivfpqfs_geometry_ok(d, nlist, M))
		throw_faiss(fn, file, "This index type is not implemented on the MI355X path yet: IndexIVFPQFastScan with d = %d, nlist = %lld, M = %d (an even "
		            "number of subquantizers, 2 to %d, nlist >= 1)", d, (long long)nlist, M, PQFS_MAX_M);
	if (metric != METRIC_L2 && metric != METRIC_IP)
		throw_faiss(fn, file, "This index type is not implemented on the MI355X path yet: IndexIVFPQFastScan with metric type %d", metric);
	if (d % M != 0)
		throw_faiss("faiss::ProductQuantizer::set_derived_values()", "faiss/impl/ProductQuantizer.cpp",
		            "Error: 'd %% M == 0' failed: The dimension of the vector (d) should be a multiple of the number of subquantizers (M)");
	return new IVFPQFSIndex(d, nlist, M, metric);
}
IndexBase *ivfpqfs_from_host(const HostIndex &h, int device) {
	CtorDevice scope(device);
	if (!h.sub || h.sub->kind != MVS_KIND_FLAT || !ivfpqfs_geometry_ok(h.d, h.nlist, h.pq_M) || h.d % h.pq_M != 0 ||
	    (h.sub->ntotal != 0 && (h.sub->ntotal != h.nlist || h.sub->d != h.d)))
		throw_faiss("mvs::ivfpqfs_from_host", __FILE__, "IVFPQFastScan image with nlist = %lld, M = %d at d = %d is not served on the MI355X path",
		            (long long)h.nlist, h.pq_M, h.d);
	auto *p = new IVFPQFSIndex(h.d, h.nlist, h.pq_M, h.metric);
	try {
		if (h.sub->ntotal > 0)
			p->coarse.quantizer->add(h.sub->ntotal, h.sub->rows.data());
		p->load_image(h);
	} catch (...) {
		delete p;
		throw;
	}
	return p;
}
bool ivfpqfs_info(const IndexBase *ix, int *M, int *nbits) {
	if (ix->kind != MVS_KIND_IVFPQFS)
		return false;
	if (M)
		*M = static_cast<const IVFPQFSIndex *>(ix)->M;
	if (nbits)
		*nbits = 4;
	return true;
}
bool ivfpqfs_get_codebooks(IndexBase *ix, float *out) {
	IVFPQFSIndex *p = as_ivfpqfs(ix);
	if (p)
		p->get_codebooks(out);
	return p != nullptr;
}
bool ivfpqfs_set_codebooks(IndexBase *ix, const float *c) {
	IVFPQFSIndex *p = as_ivfpqfs(ix);
	if (p)
		p->set_codebooks(c);
	return p != nullptr;
}

} // namespace mvs
