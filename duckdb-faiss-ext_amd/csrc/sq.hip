// csrc/sq.hip -- "SQ8" (faiss::IndexScalarQuantizer) and "IVF<n>,SQ8" (faiss::IndexIVFScalarQuantizer, an IndexIVF: the dynamic_cast of
// src/faiss_extension.cpp:675 sets nprobe on it): one byte per component, a per-dimension range learnt from min / max.
//
// Contract (include/mi355_faiss.h "8-bit scalar-quantised indexes"):
//   train   vmin[k], vdiff[k] = max - min of component k over the training rows (IVF: over their residuals x - c against the k = 1
//           centroid; the coarse centroids are what IVF<n>,Flat of the same metric learns); s[k] = vdiff[k] / 255, a[k] = vmin[k] + 0.5 s[k]
//   add     code[k] = (int)(255 * clamp((y - vmin[k]) / vdiff[k], 0, 1)), 0 where vdiff[k] == 0; y = x[k] or the residual
//   search  dec(c, k) = a[k] + (float)c * s[k]; L2: acc = fmaf(t, t, acc), t = v[k] - dec, v = x - c (IVF) or x; inner product:
//           acc = fmaf(x[k], dec, acc), IVF: + the chain <x, c>; the k best in the PURE order: distance, then probe rank, then position
//
// EVERY operation above is one IEEE f32 operation rounded on its own.  Device code is compiled with floating-point contraction on, and
// __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn are plain operators that inline INTO that mode: a[k] + c * s[k] written with them still
// becomes one fma.  The whole translation unit is therefore compiled with contraction off (the pragma below, which the compiler's default
// mode for device code honours), the rounded operations are the sq_* helpers under it, and the chains are explicit fmaf calls.
//
// SQ8 is the degenerate case of the IVF machinery: ONE list that holds every row in arrival order (the arrival-order store itself: no
// second copy), no centroid (v = x, no base), probe rank 0 for every query; (distance, rank, position) is then (distance, row).
//
// Kernels
//   sq8_minmax_kernel / sq8_minmax_fold_kernel   (csrc/sq8_kernels.h, shared with csrc/hnsw.hip's "HNSW<M>,SQ8") two-stage min / max per
//                             component over (the residuals of) a batch of training rows
//   sq8_derive_kernel         (csrc/sq8_kernels.h) vdiff, s, a from the range
//   sq8_encode_kernel         (csrc/sq8_kernels.h) residual + code, one lane per component
//   ivfpq_gather_codes / prefix / count / offsets / scatter_kernel   (csrc/ivf_units.h) list view, ordinals, pairs grouped by list
//   sq8_scan_kernel<Q, L2>    the hot path: a workgroup takes (<= Q pairs of one list, <= R positions of it).  The pairs' vectors sit in LDS
//                             interleaved [k][Q]: one broadcast 16-byte read hands a lane four pairs' values of component k.  A lane owns a
//                             row; the codes of 1024 rows travel through LDS in chunks of 32 components (coalesced 16-byte loads, rows at a
//                             pitch of 48 bytes -- an odd number of 16-byte words -- so that a lane's own 16-byte reads do not collide); one
//                             conversion and the two-operation decode per component serve all Q pairs, then one subtraction and one fmaf
//                             (L2) or one fmaf (inner product) per pair.  A value strictly below its query's bound goes to the query's
//                             bucket as (order key, ordinal)
//   pq_select_kernel          (csrc/pq_kernels.h) list + bucket sorted, the k best stay, the k-th key becomes the bound
//   sq8_emit_kernel           ordinal -> (rank, position) -> stored id (IDMap: id_map[id]), -1 / FLT_MAX padded
//
// Selection: csrc/ivfpq.hip's unit scheme as it stands -- units of (rank span, position window), ordinal = rows of the lower ranks'
// lists + position, a bucket of R entries per query, an overflowing unit scanned again in halves.  A unit of ONE rank whose list is
// longer than R is walked in windows [0, R), [R, 3R), [3R, 9R), ... (csrc/pq.hip's ranges): the first cannot overflow and leaves a bound.
#include "ivf_units.h"
#include "pq_kernels.h"
#include "sq8_kernels.h"

#include <algorithm>
#include <cstring>
#include <functional>

#pragma clang fp contract(off)

namespace mvs {

namespace {

constexpr int SQ_MAX_D = 2048;
constexpr int SQ_ROWS_PER_WG = PQ_ROWS_PER_WG; // positions of a list one scan workgroup walks = bucket entries (pq_select_kernel's pitch)
constexpr int SQ_THREADS = 1024;               // 4 waves per SIMD; a block of 1024 rows is staged at a time
constexpr int SQ_KC = 32;                      // components per staged chunk: two 16-byte words a row
constexpr int SQ_TILE_WORDS = 3;               // LDS pitch of a staged row in 16-byte words (48 bytes)
constexpr int SQ_MAX_Q = 16;

// pairs per workgroup: the pairs' vectors take Q d floats of LDS next to the 48 KB code tile and the 8 d bytes of (a, s) --
// d = 512: 32 + 48 + 4 KB; d = 2048: 64 + 48 + 16 KB of the CU's 160 KB
inline int sq_pair_block(int d) {
	return d <= 512 ? 16 : 8;
}
inline size_t sq_scan_lds(int d, int Q) {
	return (size_t)SQ_THREADS * SQ_TILE_WORDS * 16 + (size_t)d * Q * sizeof(float) + (size_t)d * 2 * sizeof(float) + (size_t)4 * SQ_MAX_Q * sizeof(float);
}


// ---------------------------------------------------------------------------------------------- scan
struct SqScan {
	const unsigned char *codes; // rows of `pitch` bytes: list-sorted (IVF) or in arrival order (SQ8)
	const long long *lids;      // their stored ids; null (SQ8): the row number
	const long long *list_off;  // [nlist + 1]
	const float *cent;          // [nlist][d]; null (SQ8): no centroid
	const float *par;           // [4][d] vmin | vdiff | a | s
	const float *xq;            // the chunk's queries [nqc][d]
	const unsigned *pref;       // the chunk's ordinal bases [nqc][np + 1]
	const int2 *pairs;          // the unit's (query, rank) pairs grouped by list
	const int *poff, *goff;     // [nlist + 1]
	const unsigned *thr;        // [nqc] bounds
	unsigned long long *bucket; // [nqc][R]
	unsigned *cnt;              // [nqc]
	int *overflow;
	const long long *idmap;
	long long id0; // SQ8: label of row 0 without an id map
	int nlist, d, pitch, np;
	long long p0, p1; // the unit's position window
	SelectorDev sel;
};

// the chains of Q pairs advance by component k: one decode, shared; V points at the pairs' values of component k
template <int Q, bool L2>
__device__ __forceinline__ void sq_step(float (&acc)[Q], const float4 *__restrict__ V, float dec) {
#pragma unroll
	for (int s4 = 0; s4 < Q / 4; ++s4) {
		const float4 v = V[s4]; // (the same address in every lane: an LDS broadcast)
		if (L2) {
			const float t0 = sq_sub(v.x, dec), t1 = sq_sub(v.y, dec), t2 = sq_sub(v.z, dec), t3 = sq_sub(v.w, dec);
			acc[4 * s4 + 0] = fmaf(t0, t0, acc[4 * s4 + 0]);
			acc[4 * s4 + 1] = fmaf(t1, t1, acc[4 * s4 + 1]);
			acc[4 * s4 + 2] = fmaf(t2, t2, acc[4 * s4 + 2]);
			acc[4 * s4 + 3] = fmaf(t3, t3, acc[4 * s4 + 3]);
		} else {
			acc[4 * s4 + 0] = fmaf(v.x, dec, acc[4 * s4 + 0]);
			acc[4 * s4 + 1] = fmaf(v.y, dec, acc[4 * s4 + 1]);
			acc[4 * s4 + 2] = fmaf(v.z, dec, acc[4 * s4 + 2]);
			acc[4 * s4 + 3] = fmaf(v.w, dec, acc[4 * s4 + 3]);
		}
	}
}

// workgroup blockIdx.x = one pair group (<= Q pairs of one list), blockIdx.y = the segment of R positions of the window
template <int Q, bool L2>
__global__ __launch_bounds__(SQ_THREADS) void sq8_scan_kernel(const SqScan a) {
	extern __shared__ __attribute__((aligned(16))) uint4 sq_lds[];
	const int tid = threadIdx.x, g = blockIdx.x;
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
	const long long s0 = a.p0 + (long long)blockIdx.y * SQ_ROWS_PER_WG;
	if (s0 >= w1)
		return; // (uniform over the workgroup: no barrier has been reached)
	const long long s1 = s0 + SQ_ROWS_PER_WG < w1 ? s0 + SQ_ROWS_PER_WG : w1;
	const int pj = a.poff[l] + (g - a.goff[l]) * Q;
	const int npg = a.poff[l + 1] - pj < Q ? a.poff[l + 1] - pj : Q; // pairs of this group, >= 1
	const int d = a.d;
	// LDS: code tile [1024][3] words | V [d][Q] | (a, s) [d] | base [16] | query [16] | ordinal base [16] | bound [16]
	uint4 *tile = sq_lds;
	float *V = reinterpret_cast<float *>(tile + SQ_THREADS * SQ_TILE_WORDS);
	float2 *AS = reinterpret_cast<float2 *>(V + (size_t)d * Q);
	float *s_base = reinterpret_cast<float *>(AS + d);
	int *s_q = reinterpret_cast<int *>(s_base + SQ_MAX_Q);
	unsigned *s_ord = reinterpret_cast<unsigned *>(s_q + SQ_MAX_Q);
	unsigned *s_thr = s_ord + SQ_MAX_Q;
	const float *cl = a.cent ? a.cent + (size_t)l * d : nullptr;
	if (tid < Q) {
		int q = 0;
		unsigned ord = 0u, th = 0u; // (bound 0: no key is below it -- a slot without a pair admits nothing)
		float acc = 0.f;
		if (tid < npg) {
			const int2 p = a.pairs[pj + tid];
			q = p.x;
			ord = a.pref[(size_t)p.x * (a.np + 1) + p.y];
			th = a.thr[q];
			if (!L2 && cl) { // base = the ip chain <x, c>, k ascending
				const float *xv = a.xq + (size_t)p.x * d;
				for (int k = 0; k < d; ++k)
					acc = fmaf(xv[k], cl[k], acc);
			}
		}
		s_q[tid] = q, s_ord[tid] = ord, s_thr[tid] = th, s_base[tid] = acc;
	}
	__syncthreads();
	for (int i = tid; i < Q * d; i += SQ_THREADS) {
		const int s = i / d, k = i - s * d;
		float v = 0.f;
		if (s < npg) {
			v = a.xq[(size_t)s_q[s] * d + k];
			if (L2 && cl)
				v = sq_sub(v, cl[k]);
		}
		V[k * Q + s] = v;
	}
	for (int k = tid; k < d; k += SQ_THREADS)
		AS[k] = make_float2(a.par[2 * d + k], a.par[3 * d + k]);
	const int words = a.pitch >> 4;
	for (long long pb = s0; pb < s1; pb += SQ_THREADS) { // (uniform trip count: the barriers below are reached by every lane)
		const long long pos = pb + tid;
		float acc[Q];
#pragma unroll
		for (int s = 0; s < Q; ++s)
			acc[s] = 0.f;
		for (int k0 = 0; k0 < d; k0 += SQ_KC) {
			__syncthreads(); // (V and (a, s) are written; the previous chunk's tile has been read)
#pragma unroll
			for (int i = 0; i < 2; ++i) { // 1024 rows x 2 words: four lanes read a row's 32 bytes ... 64 contiguous bytes at d = 32
				const int idx = tid + i * SQ_THREADS, r = idx >> 1, w = idx & 1;
				const int gw = (k0 >> 4) + w;
				uint4 cw = make_uint4(0u, 0u, 0u, 0u);
				if (pb + r < s1 && gw < words)
					cw = reinterpret_cast<const uint4 *>(a.codes + (size_t)(lb + pb + r) * a.pitch)[gw];
				tile[r * SQ_TILE_WORDS + w] = cw;
			}
			__syncthreads();
#pragma unroll
			for (int w = 0; w < 2; ++w) {
				const int kw = k0 + w * 16;
				if (kw >= d)
					break;
				const uint4 cw = tile[tid * SQ_TILE_WORDS + w];
#pragma unroll 1
				for (int j = 0; j < 4; ++j) { // one 32-bit word at a time: the chains of 16 pairs and four components' values fill the registers
					const unsigned wj = j == 0 ? cw.x : (j == 1 ? cw.y : (j == 2 ? cw.z : cw.w));
#pragma unroll
					for (int b = 0; b < 4; ++b) {
						const int k = kw + 4 * j + b;
						if (k < d) { // (the padded components of the row's last word do not enter the chain)
							const float c = (float)((wj >> (b * 8)) & 255u);
							const float2 as = AS[k];
							sq_step<Q, L2>(acc, reinterpret_cast<const float4 *>(V + (size_t)k * Q), sq_add(as.x, sq_mul(c, as.y)));
						}
					}
				}
			}
		}
		if (pos >= s1)
			continue;
		if (a.sel.kind != MVS_SEL_NONE) {
			const long long id = a.lids ? a.lids[lb + pos] : lb + pos;
			if (!pq_sel_member(a.sel, a.idmap ? a.idmap[id] : (a.lids ? id : id + a.id0)))
				continue;
		}
#pragma unroll
		for (int s = 0; s < Q; ++s) {
			const float v = !L2 && cl ? sq_add(s_base[s], acc[s]) : acc[s];
			const unsigned key = pq_key(v, L2 ? 0 : 1);
			if (key < s_thr[s]) {
				const int q = s_q[s];
				const unsigned at = atomicAdd(&a.cnt[q], 1u);
				if (at < (unsigned)SQ_ROWS_PER_WG)
					a.bucket[(size_t)q * SQ_ROWS_PER_WG + at] = ((unsigned long long)key << 32) | (unsigned long long)(s_ord[s] + (unsigned)pos);
				else
					*a.overflow = 1;
			}
		}
	}
}

// ---------------------------------------------------------------------------------------------- emit
__global__ __launch_bounds__(256) void sq8_emit_kernel(const unsigned long long *__restrict__ list, const int *__restrict__ len, int k, long long nqc,
                                                       int descending, const long long *__restrict__ cI, int np, const unsigned *__restrict__ pref,
                                                       const long long *__restrict__ list_off, const long long *__restrict__ lids, long long id0,
                                                       const long long *__restrict__ idmap, float *__restrict__ D, long long *__restrict__ I) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nqc * k)
		return;
	const long long q = i / k;
	const int s = (int)(i - q * k);
	if (s < len[q]) {
		const unsigned long long e = list[i];
		const unsigned ord = (unsigned)(e & 0xFFFFFFFFull);
		const unsigned *pq = pref + q * (np + 1);
		int lo = 0, hi = np; // pq[lo] <= ord < pq[hi]: the rank whose list holds the ordinal
		while (hi - lo > 1) {
			const int mid = (lo + hi) >> 1;
			if (pq[mid] <= ord)
				lo = mid;
			else
				hi = mid;
		}
		const long long row = list_off[cI[q * np + lo]] + (ord - pq[lo]);
		const long long id = lids ? lids[row] : row;
		D[i] = pq_unkey((unsigned)(e >> 32), descending);
		I[i] = idmap ? idmap[id] : (lids ? id : id + id0);
	} else {
		D[i] = descending ? -FLT_MAX : FLT_MAX;
		I[i] = -1;
	}
}

// ---------------------------------------------------------------------------------------------- index
class SQIndex : public IndexBase {
public:
	FlatIndex *quantizer = nullptr; // IVF: owned, nlist centroids; SQ8: none
	const bool ivf;
	const int64_t nlist; // SQ8: the one list
	const int pitch;     // code bytes per row in the stores, d rounded up to 16
	int64_t nprobe = 1;
	bool have_par = false;
	float *d_par = nullptr;           // [4][d] vmin | vdiff | a | s
	unsigned char *d_codes = nullptr; // [cap][pitch] arrival order
	int64_t cap = 0;
	std::vector<int32_t> assign_h; // IVF only
	std::vector<int64_t> ids_h;    // IVF only
	// the list view, rebuilt lazily (SQ8: the arrival-order store is the list)
	bool dirty = true, cent_dirty = true;
	std::vector<int64_t> list_off, sid_h, top_rows; // top_rows[i]: rows of the i largest lists together
	int64_t nsorted = 0, max_list = 0;
	DevBuf lcodes, lids, list_off_dev, cent_dev;
	DevBuf ws_add, ws_lab, ws_part, ws_cD, ws_cI, ws_pref, ws_pairs, ws_grp, ws_bucket, ws_list, ws_ctl;
	int *h_flag = nullptr; // pinned
	SelectorHolder selector;
	int64_t last_launches = 0, last_rescans = 0;

	SQIndex(int d_, int64_t nlist_, int metric_)
	    : IndexBase(nlist_ > 0 ? MVS_KIND_IVFSQ : MVS_KIND_SQ, d_, metric_), ivf(nlist_ > 0), nlist(nlist_ > 0 ? nlist_ : 1), pitch((d_ + 15) / 16 * 16) {
		if (metric != METRIC_L2 && metric != METRIC_IP)
			throw_faiss("mvs::SQIndex", __FILE__, "metric type %d is not implemented on the MI355X path", metric);
		if (ivf)
			quantizer = new FlatIndex(d, metric);
		is_trained = false;
	}
	~SQIndex() override {
		(void)hipSetDevice(device);
		if (stream)
			(void)hipStreamSynchronize(stream);
		free_device();
		delete quantizer;
	}
	void free_device() {
		if (d_par)
			(void)hipFree(d_par);
		if (d_codes)
			(void)hipFree(d_codes);
		if (h_flag)
			(void)hipHostFree(h_flag);
		d_par = nullptr, d_codes = nullptr, h_flag = nullptr, cap = 0;
		for (DevBuf *b : {&lcodes, &lids, &list_off_dev, &cent_dev, &ws_add, &ws_lab, &ws_part, &ws_cD, &ws_cI, &ws_pref, &ws_pairs, &ws_grp, &ws_bucket,
		                  &ws_list, &ws_ctl})
			b->release();
		selector.buf.release();
		dirty = cent_dirty = true;
	}
	void adopt_tuning(const Tuning &t) override {
		tune_ = t;
		if (quantizer)
			quantizer->adopt_tuning(t);
	}

	// ------------------------------------------------------------------------------------------ train
	void check_empty_for_training() const {
		if (ntotal > 0)
			throw_faiss("mvs::SQIndex::train", __FILE__, "the index already holds %lld rows encoded with its range%s: "
			            "training again is only possible while it is empty", (long long)ntotal, ivf ? " and centroids" : "");
	}
	void update_trained() {
		is_trained = have_par && (!ivf || quantizer->ntotal == nlist);
	}
	void ensure_par() {
		if (!d_par)
			MVS_HIP(hipMalloc((void **)&d_par, (size_t)4 * d * sizeof(float)));
	}
	void derive(bool from_range) { // (on `stream`)
		hipLaunchKernelGGL(sq8_derive_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, stream, d_par, d, from_range ? 1 : 0);
		MVS_HIP(hipGetLastError());
		MVS_HIP(hipStreamSynchronize(stream));
		have_par = true;
		update_trained();
	}
	void set_coarse(const float *c) {
		use_device();
		check_empty_for_training();
		quantizer->reset();
		quantizer->add(nlist, c);
		cent_dirty = true;
		update_trained();
	}
	void set_trained(const float *t) { // [2][d] vmin | vdiff
		use_device();
		check_empty_for_training();
		ensure_par();
		MVS_HIP(hipMemcpyAsync(d_par, t, (size_t)2 * d * sizeof(float), hipMemcpyHostToDevice, stream));
		derive(false);
	}
	void get_trained(float *out) {
		use_device();
		if (!have_par)
			throw_faiss("mvs::SQIndex::get_trained", __FILE__, "the index has no trained range yet");
		MVS_HIP(hipStreamSynchronize(stream));
		MVS_HIP(hipMemcpy(out, d_par, (size_t)2 * d * sizeof(float), hipMemcpyDeviceToHost));
	}
	void get_coarse(float *out) {
		use_device();
		HostIndex h;
		quantizer->to_host(h);
		memcpy(out, h.rows.data(), h.rows.size() * sizeof(float));
	}
	const float *centroids_dev() { // [nlist][d] row-major copy of the quantiser's rows (on `stream`); null for SQ8
		if (!ivf)
			return nullptr;
		if (cent_dirty) {
			std::vector<float> c((size_t)nlist * d);
			get_coarse(c.data());
			cent_dev.reserve(c.size() * sizeof(float));
			MVS_HIP(hipMemcpyAsync(cent_dev.p, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice, stream));
			MVS_HIP(hipStreamSynchronize(stream));
			cent_dirty = false;
		}
		return (const float *)cent_dev.p;
	}
	// the quantiser's k = 1 label of n device rows (on `stream`), the call add and train share
	void assign_device(int64_t n, const float *d_x, float *d_D, int64_t *d_I) {
		if (!quantizer->coarse_topk(n, d_x, 1, d_D, d_I, stream, false))
			quantizer->search_device(n, d_x, 1, d_D, d_I, nullptr, stream);
		use_device();
	}
	void train(int64_t n, const float *x) override {
		use_device();
		check_empty_for_training();
		n = std::max<int64_t>(n, 0);
		CtorDevice scope(device);
		if (ivf) { // the coarse centroids: IVF<n>,Flat of the same metric (spherical under inner product, as there)
			std::unique_ptr<IndexBase> iv(make_ivf_index(d, "IVF" + std::to_string(nlist) + ",Flat", metric));
			iv->adopt_tuning(tune_);
			iv->train(n, x);
			std::vector<float> cent((size_t)nlist * d);
			ivf_get_centroids(iv.get(), cent.data());
			have_par = false;
			set_coarse(cent.data());
		}
		if (n <= 0)
			throw_faiss("virtual void faiss::ScalarQuantizer::train(size_t, const float*)", "faiss/impl/ScalarQuantizer.cpp",
			            "Error: 'n > 0' failed: the range of a scalar quantizer needs at least one training row");
		// min / max per component over the rows (IVF: over every row's residual against its k = 1 centroid), batch by batch on the device
		ensure_par();
		const int64_t bs = 65536;
		const int64_t nb_max = std::min(bs, n);
		const int chunks_max = (int)((nb_max + SQ_MINMAX_ROWS - 1) / SQ_MINMAX_ROWS);
		ws_add.reserve((size_t)nb_max * d * sizeof(float));
		ws_lab.reserve((size_t)nb_max * (sizeof(float) + sizeof(int64_t)));
		ws_part.reserve((size_t)chunks_max * 2 * d * sizeof(float));
		const float *d_cent = centroids_dev();
		for (int64_t i0 = 0; i0 < n; i0 += bs) {
			const int64_t nb = std::min(bs, n - i0);
			MVS_HIP(hipMemcpyAsync(ws_add.p, x + i0 * d, (size_t)nb * d * sizeof(float), hipMemcpyHostToDevice, stream));
			int64_t *d_lab = nullptr;
			if (ivf) {
				d_lab = (int64_t *)ws_lab.p;
				assign_device(nb, (const float *)ws_add.p, (float *)(d_lab + nb), d_lab);
			}
			const int chunks = (int)((nb + SQ_MINMAX_ROWS - 1) / SQ_MINMAX_ROWS);
			const unsigned gk = (unsigned)((d + 255) / 256);
			hipLaunchKernelGGL(sq8_minmax_kernel, dim3(gk, (unsigned)chunks), dim3(256), 0, stream, (const float *)ws_add.p, (long long)nb, d,
			                   (const long long *)d_lab, d_cent, (long long)nlist, (float *)ws_part.p);
			hipLaunchKernelGGL(sq8_minmax_fold_kernel, dim3(gk), dim3(256), 0, stream, (const float *)ws_part.p, chunks, d, d_par, i0 == 0 ? 1 : 0);
			MVS_HIP(hipGetLastError());
			MVS_HIP(hipStreamSynchronize(stream)); // (ws_add is filled again)
		}
		derive(true);
	}

	// ------------------------------------------------------------------------------------------ add
	void grow(int64_t need) {
		if (need <= cap)
			return;
		int64_t nc = cap ? cap : 4096;
		while (nc < need)
			nc = nc + nc / 2 + 4096;
		unsigned char *nb = nullptr;
		MVS_HIP(hipMalloc((void **)&nb, (size_t)nc * pitch));
		MVS_HIP(hipMemsetAsync(nb, 0, (size_t)nc * pitch, stream));
		if (ntotal > 0)
			MVS_HIP(hipMemcpyAsync(nb, d_codes, (size_t)ntotal * pitch, hipMemcpyDeviceToDevice, stream));
		MVS_HIP(hipStreamSynchronize(stream));
		if (d_codes)
			MVS_HIP(hipFree(d_codes));
		d_codes = nb;
		cap = nc;
	}
	void set_label_offset(int64_t off) override {
		if (ivf && ntotal > 0 && off != label_offset)
			throw_faiss("mvs::SQIndex::set_label_offset", __FILE__, "the label offset of an IVF index must be set before rows are added");
		label_offset = off;
	}
	void check_trained_for_add() const {
		if (!is_trained)
			throw_faiss(ivf ? "virtual void faiss::IndexIVFScalarQuantizer::add_core(...)" : "virtual void faiss::IndexFlatCodes::add(...)",
			            ivf ? "faiss/IndexScalarQuantizer.cpp" : "faiss/IndexFlatCodes.cpp", "Error: 'is_trained' failed");
	}
	// d_x: [n][d] rows on the device, in `stream` order; ids (host) may be null
	void add_core_device(int64_t n, const float *d_x, const int64_t *ids_host) {
		check_trained_for_add();
		if (ntotal + n > (int64_t)0x7fffffff - 1024)
			throw_faiss("mvs::SQIndex::add", __FILE__, "a single-device index holds at most 2^31 rows");
		grow(ntotal + n);
		const int64_t bs = 65536; // IndexIVF::add_with_ids block size
		std::vector<int64_t> lab;
		if (ivf) {
			ws_lab.reserve((size_t)std::min(bs, n) * (sizeof(float) + sizeof(int64_t)));
			lab.resize((size_t)std::min(bs, n));
			assign_h.reserve((size_t)(ntotal + n));
			ids_h.reserve((size_t)(ntotal + n));
		}
		const float *d_cent = centroids_dev();
		for (int64_t i0 = 0; i0 < n; i0 += bs) {
			const int64_t nb = std::min(bs, n - i0);
			int64_t *d_lab = nullptr;
			if (ivf) {
				d_lab = (int64_t *)ws_lab.p;
				assign_device(nb, d_x + i0 * d, (float *)(d_lab + nb), d_lab);
				MVS_HIP(hipMemcpyAsync(lab.data(), d_lab, (size_t)nb * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
			}
			const long long tot = nb * d;
			hipLaunchKernelGGL(sq8_encode_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, d_x + i0 * d, (long long)nb, d,
			                   (const long long *)d_lab, d_cent, (long long)nlist, (const float *)d_par, d_codes, pitch, (long long)(ntotal + i0));
			MVS_HIP(hipGetLastError());
			MVS_HIP(hipStreamSynchronize(stream));
			if (ivf)
				for (int64_t i = 0; i < nb; i++) {
					const int64_t l = lab[(size_t)i];
					assign_h.push_back(l >= 0 && l < nlist ? (int32_t)l : -1);
					ids_h.push_back(ids_host ? ids_host[i0 + i] : label_offset + ntotal + i0 + i);
				}
		}
		ntotal += n;
		dirty = true;
	}
	void add_host(int64_t n, const float *x, const int64_t *ids) {
		use_device();
		if (n <= 0)
			return;
		check_trained_for_add(); // (before the rows travel)
		const int64_t bs = 1 << 20; // rows staged at a time: the index is wanted for databases larger than a staging buffer should be
		ws_add.reserve((size_t)std::min(bs, n) * d * sizeof(float));
		for (int64_t i0 = 0; i0 < n; i0 += bs) {
			const int64_t nb = std::min(bs, n - i0);
			MVS_HIP(hipMemcpyAsync(ws_add.p, x + i0 * d, (size_t)nb * d * sizeof(float), hipMemcpyHostToDevice, stream));
			add_core_device(nb, (const float *)ws_add.p, ids ? ids + i0 : nullptr);
		}
	}
	void add(int64_t n, const float *x) override {
		add_host(n, x, nullptr);
	}
	void add_with_ids(int64_t n, const float *x, const int64_t *ids) override {
		if (!ivf)
			return IndexBase::add_with_ids(n, x, ids); // "add_with_ids not implemented for this type of index"
		add_host(n, x, ids);
	}
	void add_device(int64_t n, const float *d_x, hipStream_t st) override {
		use_device();
		if (n <= 0)
			return;
		stream_wait(stream, st);
		add_core_device(n, d_x, nullptr);
	}
	void add_with_ids_device(int64_t n, const float *d_x, const int64_t *d_ids, hipStream_t st) override {
		if (!ivf)
			return IndexBase::add_with_ids_device(n, d_x, d_ids, st);
		use_device();
		if (n <= 0)
			return;
		stream_wait(stream, st);
		std::vector<int64_t> ids((size_t)n);
		MVS_HIP(hipMemcpy(ids.data(), d_ids, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
		add_core_device(n, d_x, ids.data());
	}

	// ------------------------------------------------------------------------------------------ list view
	// IVF: rows grouped by list, arrival order inside a list (ArrayInvertedLists semantics), codes gathered on the device.
	// SQ8: one list = the arrival-order store
	void build_lists() {
		if (!dirty)
			return;
		list_off.assign((size_t)nlist + 1, 0);
		if (!ivf) {
			list_off[1] = ntotal;
			max_list = nsorted = ntotal;
			top_rows.assign(1, ntotal);
		} else {
			for (int64_t i = 0; i < ntotal; i++)
				if (assign_h[(size_t)i] >= 0)
					list_off[(size_t)assign_h[(size_t)i] + 1]++;
			max_list = 0;
			top_rows.assign((size_t)nlist, 0);
			for (int64_t l = 0; l < nlist; l++) {
				top_rows[(size_t)l] = list_off[(size_t)l + 1];
				max_list = std::max(max_list, list_off[(size_t)l + 1]);
			}
			std::sort(top_rows.begin(), top_rows.end(), std::greater<int64_t>());
			for (int64_t l = 1; l < nlist; l++)
				top_rows[(size_t)l] += top_rows[(size_t)l - 1];
			for (int64_t l = 0; l < nlist; l++)
				list_off[(size_t)l + 1] += list_off[(size_t)l];
			nsorted = list_off[(size_t)nlist];
			std::vector<int64_t> cursor(list_off.begin(), list_off.end() - 1);
			std::vector<int32_t> perm((size_t)nsorted);
			sid_h.assign((size_t)nsorted, 0);
			for (int64_t i = 0; i < ntotal; i++) {
				const int32_t l = assign_h[(size_t)i];
				if (l < 0)
					continue;
				const int64_t p = cursor[(size_t)l]++;
				perm[(size_t)p] = (int32_t)i;
				sid_h[(size_t)p] = ids_h[(size_t)i];
			}
			lcodes.reserve((size_t)std::max<int64_t>(nsorted, 1) * pitch);
			lids.reserve((size_t)std::max<int64_t>(nsorted, 1) * sizeof(int64_t));
			DevBuf dperm;
			dperm.reserve((size_t)std::max<int64_t>(nsorted, 1) * sizeof(int32_t));
			if (nsorted > 0) {
				MVS_HIP(hipMemcpyAsync(dperm.p, perm.data(), (size_t)nsorted * sizeof(int32_t), hipMemcpyHostToDevice, stream));
				MVS_HIP(hipMemcpyAsync(lids.p, sid_h.data(), (size_t)nsorted * sizeof(int64_t), hipMemcpyHostToDevice, stream));
				const int words = pitch / 16;
				const long long tot = nsorted * words;
				hipLaunchKernelGGL(ivfpq_gather_codes_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, (const uint4 *)d_codes,
				                   (const int *)dperm.p, (long long)nsorted, words, (uint4 *)lcodes.p);
				MVS_HIP(hipGetLastError());
			}
			MVS_HIP(hipStreamSynchronize(stream)); // (dperm is released)
		}
		list_off_dev.reserve(list_off.size() * sizeof(int64_t));
		MVS_HIP(hipMemcpyAsync(list_off_dev.p, list_off.data(), list_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
		MVS_HIP(hipStreamSynchronize(stream));
		dirty = false;
	}
	const unsigned char *list_codes() const {
		return ivf ? (const unsigned char *)lcodes.p : d_codes;
	}
	int64_t list_size(int64_t l) {
		use_device();
		if (l < 0 || l >= nlist)
			throw_faiss("mvs::SQIndex::list_size", __FILE__, "list %lld is outside [0, %lld)", (long long)l, (long long)nlist);
		build_lists();
		return list_off[(size_t)l + 1] - list_off[(size_t)l];
	}
	void get_list(int64_t l, int64_t *ids, uint8_t *codes) {
		const int64_t n = list_size(l), b = list_off[(size_t)l];
		if (n <= 0)
			return;
		if (ids)
			memcpy(ids, &sid_h[(size_t)b], (size_t)n * sizeof(int64_t));
		if (codes)
			MVS_HIP(hipMemcpy2D(codes, (size_t)d, list_codes() + (size_t)b * pitch, (size_t)pitch, (size_t)d, (size_t)n, hipMemcpyDeviceToHost));
	}
	void get_codes(int64_t row0, int64_t n, uint8_t *out) { // SQ8: rows of the arrival-order store
		use_device();
		if (row0 < 0 || n < 0 || row0 + n > ntotal)
			throw_faiss("mvs::SQIndex::get_codes", __FILE__, "rows [%lld, %lld) are outside the index (ntotal %lld)", (long long)row0,
			            (long long)(row0 + n), (long long)ntotal);
		MVS_HIP(hipStreamSynchronize(stream));
		if (n > 0)
			MVS_HIP(hipMemcpy2D(out, (size_t)d, d_codes + (size_t)row0 * pitch, (size_t)pitch, (size_t)d, (size_t)n, hipMemcpyDeviceToHost));
	}

	// ------------------------------------------------------------------------------------------ search
	struct Chunk { // one chunk of queries: device state of its selection, the scan's fixed arguments
		int64_t nqc;
		int k, Q, np;
		const int64_t *cI;
		unsigned long long *list;
		int *len, *gcnt, *gcur, *poff, *goff;
		SqScan a;
	};
	// the rows one query can send to its bucket from a unit, at most
	int64_t unit_rows(int ra, int rb, int64_t p0, int64_t p1) const {
		if (rb - ra == 1)
			return std::min(max_list, p1) - p0;
		return top_rows[(size_t)std::min<int64_t>(rb - ra, nlist) - 1];
	}
	void launch_scan(Chunk &c, int ra, int rb, int64_t p0, int64_t p1) {
		const int Q = c.Q, span = rb - ra;
		const int64_t npairs = c.nqc * span;
		// the unit's pairs grouped by list: count, offsets, scatter
		MVS_HIP(hipMemsetAsync(c.gcnt, 0, (size_t)2 * nlist * sizeof(int), stream));
		const dim3 pgrid((unsigned)((npairs + 255) / 256));
		hipLaunchKernelGGL(ivfpq_count_kernel, pgrid, dim3(256), 0, stream, (const long long *)c.cI, (long long)c.nqc, c.np, ra, rb,
		                   (const long long *)list_off_dev.p, (long long)nlist, (long long)p0, c.gcnt);
		hipLaunchKernelGGL(ivfpq_offsets_kernel, dim3(1), dim3(1024), 0, stream, (const int *)c.gcnt, (int)nlist, Q, c.poff, c.goff);
		hipLaunchKernelGGL(ivfpq_scatter_kernel, pgrid, dim3(256), 0, stream, (const long long *)c.cI, (long long)c.nqc, c.np, ra, rb,
		                   (const long long *)list_off_dev.p, (long long)nlist, (long long)p0, (const int *)c.poff, c.gcur, (int2 *)ws_pairs.p);
		MVS_HIP(hipGetLastError());
		// pair groups: sum over lists of ceil(pairs / Q) <= pairs / Q + lists that have pairs; segments of R positions of the window
		const int64_t gx = npairs / Q + 1 + std::min<int64_t>(nlist, npairs);
		const int64_t gy = (std::min(max_list, p1) - p0 + SQ_ROWS_PER_WG - 1) / SQ_ROWS_PER_WG;
		const dim3 grid((unsigned)gx, (unsigned)gy);
		const size_t lds = sq_scan_lds(d, Q);
		c.a.p0 = p0, c.a.p1 = p1;
		begin_kernel_timing(stream);
#define SQ_LAUNCH_SCAN(QQ, LL)                                                                                                                      \
	do {                                                                                                                                            \
		ensure_dynamic_lds((const void *)sq8_scan_kernel<QQ, LL>, lds);                                                                             \
		hipLaunchKernelGGL((sq8_scan_kernel<QQ, LL>), grid, dim3(SQ_THREADS), lds, stream, c.a);                                                    \
	} while (0)
		const bool l2 = metric == METRIC_L2;
		if (Q == 16 && l2)
			SQ_LAUNCH_SCAN(16, true);
		else if (Q == 16)
			SQ_LAUNCH_SCAN(16, false);
		else if (l2)
			SQ_LAUNCH_SCAN(8, true);
		else
			SQ_LAUNCH_SCAN(8, false);
#undef SQ_LAUNCH_SCAN
		MVS_HIP(hipGetLastError());
		end_kernel_timing(stream);
		const double rows = (double)unit_rows(ra, rb, p0, p1);
		set_kinfo("sq8_scan_kernel", (double)c.nqc * rows * d * (l2 ? 3.0 : 2.0), (double)c.nqc * rows * d / Q, (int)(gx * gy), SQ_THREADS, (int)lds, (int)gy);
		++last_launches;
	}
	// ranks [ra, rb), positions [p0, p1) of their lists, into every list of the chunk
	void scan_unit(Chunk &c, int ra, int rb, int64_t p0, int64_t p1) {
		launch_scan(c, ra, rb, p0, p1);
		if (unit_rows(ra, rb, p0, p1) > SQ_ROWS_PER_WG) { // (a unit of at most R rows per query cannot overflow a bucket of R entries)
			MVS_HIP(hipMemcpyAsync(h_flag, c.a.overflow, sizeof(int), hipMemcpyDeviceToHost, stream));
			MVS_HIP(hipStreamSynchronize(stream));
			if (*h_flag) { // some bucket overflowed: nothing of this unit is merged; its two halves one after the other
				MVS_HIP(hipMemsetAsync(c.a.cnt, 0, (size_t)c.nqc * sizeof(unsigned), stream));
				MVS_HIP(hipMemsetAsync(c.a.overflow, 0, sizeof(int), stream));
				++last_rescans;
				if (rb - ra > 1) {
					const int mid = ra + (rb - ra) / 2;
					scan_unit(c, ra, mid, p0, p1);
					scan_unit(c, mid, rb, p0, p1);
				} else {
					const int64_t w1 = std::min(max_list, p1);
					const int64_t mid = p0 + ((w1 - p0) / 2 + SQ_ROWS_PER_WG - 1) / SQ_ROWS_PER_WG * SQ_ROWS_PER_WG;
					scan_unit(c, ra, rb, p0, mid);
					scan_unit(c, ra, rb, mid, w1);
				}
				return;
			}
		}
		int P = 1;
		while (P < c.k + SQ_ROWS_PER_WG)
			P <<= 1;
		const size_t lds = (size_t)P * sizeof(unsigned long long);
		ensure_dynamic_lds((const void *)pq_select_kernel, lds);
		hipLaunchKernelGGL(pq_select_kernel, dim3((unsigned)c.nqc), dim3(1024), lds, stream, c.list, c.len, c.k, (const unsigned long long *)c.a.bucket,
		                   c.a.cnt, const_cast<unsigned *>(c.a.thr));
		MVS_HIP(hipGetLastError());
	}
	void search_mapped(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, const int64_t *d_idmap,
	                   hipStream_t st) override {
		use_device();
		const char *fn = ivf ? "virtual void faiss::IndexIVF::search(...) const" : "virtual void faiss::IndexFlatCodes::search(...) const";
		const char *file = ivf ? "faiss/IndexIVF.cpp" : "faiss/IndexFlatCodes.cpp";
		if (k <= 0)
			throw_faiss(fn, file, "Error: 'k > 0' failed");
		if (k > PQ_MAX_K)
			throw_faiss("mvs::SQIndex::search", __FILE__, "k = %lld is beyond the largest k the SQ8 index serves on the MI355X path (%d)", (long long)k,
			            PQ_MAX_K);
		if (!is_trained)
			throw_faiss(fn, file, "Error: 'is_trained' failed");
		if (nq <= 0)
			return;
		int64_t np = 1;
		if (ivf) {
			np = params && params->nprobe > 0 ? params->nprobe : nprobe;
			np = std::min(np, nlist); // IndexIVF::search: nprobe = min(nlist, params->nprobe)
			if (np <= 0)
				throw_faiss(fn, file, "Error: 'nprobe > 0' failed");
		}
		stream_wait(stream, st); // our stream carries the adds and the list view; the caller's the queries
		build_lists();
		const float *d_cent = centroids_dev();
		const int Q = sq_pair_block(d);
		// 1. the probed lists of the whole batch (SQ8: list 0 at rank 0), the ordinal bases
		ws_cI.reserve((size_t)nq * np * sizeof(int64_t));
		ws_pref.reserve((size_t)nq * (np + 1) * sizeof(unsigned));
		if (nsorted > 0) {
			if (ivf) {
				ws_cD.reserve((size_t)nq * np * sizeof(float));
				if (!quantizer->coarse_topk(nq, d_x, np, (float *)ws_cD.p, (int64_t *)ws_cI.p, stream, false))
					quantizer->search_device(nq, d_x, np, (float *)ws_cD.p, (int64_t *)ws_cI.p, nullptr, stream);
				use_device();
			} else {
				MVS_HIP(hipMemsetAsync(ws_cI.p, 0, (size_t)nq * sizeof(int64_t), stream));
			}
			hipLaunchKernelGGL(ivfpq_prefix_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, (const long long *)ws_cI.p, (long long)nq,
			                   (int)np, (const long long *)list_off_dev.p, (long long)nlist, (unsigned *)ws_pref.p);
			MVS_HIP(hipGetLastError());
		}
		// 2. queries per chunk: buckets <= 256 MB
		const int64_t nqc_max = std::min<int64_t>(nq, (int64_t)(PQ_BUCKET_SCRATCH / ((size_t)SQ_ROWS_PER_WG * sizeof(unsigned long long))));
		int np_span = 1; // the widest rank span a unit can have
		for (int ra = 0, rb = 1; ra < np; ra = rb, rb = (int)std::min<int64_t>(np, 3 * (int64_t)rb))
			np_span = std::max(np_span, rb - ra);
		ws_bucket.reserve((size_t)nqc_max * SQ_ROWS_PER_WG * sizeof(unsigned long long));
		ws_list.reserve((size_t)nqc_max * k * sizeof(unsigned long long));
		ws_pairs.reserve((size_t)nqc_max * np_span * sizeof(int2));
		ws_grp.reserve((size_t)(4 * nlist + 2) * sizeof(int)); // cnt [nlist] | cur [nlist] | poff [nlist + 1] | goff [nlist + 1]
		// control block: len [nqc] | cnt [nqc] | overflow (+ pad) | thr [nqc]
		const size_t ctl_zero = (size_t)(2 * nqc_max + 4) * sizeof(int);
		ws_ctl.reserve(ctl_zero + (size_t)nqc_max * sizeof(unsigned));
		if (!h_flag)
			MVS_HIP(hipHostMalloc((void **)&h_flag, sizeof(int), hipHostMallocDefault));
		Chunk c;
		c.k = (int)k, c.Q = Q, c.np = (int)np;
		c.list = (unsigned long long *)ws_list.p;
		c.len = (int *)ws_ctl.p;
		c.gcnt = (int *)ws_grp.p;
		c.gcur = c.gcnt + nlist;
		c.poff = c.gcur + nlist;
		c.goff = c.poff + nlist + 1;
		SqScan &a = c.a;
		a.codes = list_codes();
		a.lids = ivf ? (const long long *)lids.p : nullptr;
		a.list_off = (const long long *)list_off_dev.p;
		a.cent = d_cent;
		a.par = d_par;
		a.pairs = (const int2 *)ws_pairs.p;
		a.poff = c.poff, a.goff = c.goff;
		a.bucket = (unsigned long long *)ws_bucket.p;
		a.cnt = (unsigned *)ws_ctl.p + nqc_max;
		a.overflow = (int *)ws_ctl.p + 2 * nqc_max;
		a.thr = (unsigned *)((char *)ws_ctl.p + ctl_zero);
		a.idmap = (const long long *)d_idmap;
		a.id0 = label_offset;
		a.nlist = (int)nlist, a.d = d, a.pitch = pitch, a.np = (int)np;
		a.p0 = 0, a.p1 = 0;
		a.sel = selector.upload(params, stream);
		last_launches = last_rescans = 0;
		memset(&kinfo, 0, sizeof kinfo);
		for (int64_t q0 = 0; q0 < nq; q0 += nqc_max) {
			c.nqc = std::min(nqc_max, nq - q0);
			c.cI = (const int64_t *)ws_cI.p + q0 * np;
			a.xq = d_x + q0 * d;
			a.pref = (const unsigned *)ws_pref.p + q0 * (np + 1);
			MVS_HIP(hipMemsetAsync(ws_ctl.p, 0, ctl_zero, stream));
			MVS_HIP(hipMemsetAsync(const_cast<unsigned *>(a.thr), 0xFF, (size_t)nqc_max * sizeof(unsigned), stream)); // (every key is below it: an open list admits all)
			if (nsorted > 0)
				for (int ra = 0, rb = 1; ra < np; ra = rb, rb = (int)std::min<int64_t>(np, 3 * (int64_t)rb)) {
					if (rb - ra > 1) {
						scan_unit(c, ra, rb, 0, max_list);
						continue;
					}
					// one rank: windows [0, R), [R, 3R), [3R, 9R), ... -- positions ascend, so the ordinals still do
					for (int64_t p0 = 0, p1 = SQ_ROWS_PER_WG; p0 < max_list; p0 = p1, p1 = 3 * p1)
						scan_unit(c, ra, rb, p0, std::min(p1, max_list));
				}
			const int64_t tot = c.nqc * k;
			hipLaunchKernelGGL(sq8_emit_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, (const unsigned long long *)c.list,
			                   (const int *)c.len, c.k, (long long)c.nqc, metric == METRIC_IP ? 1 : 0, (const long long *)c.cI, (int)np, a.pref,
			                   (const long long *)list_off_dev.p, a.lids, (long long)label_offset,
			                   raw_labels ? nullptr : (const long long *)d_idmap, d_D + q0 * k, // (raw_labels: csrc/index.h; the offset of a refine base stays 0)
			                   (long long *)(d_I + q0 * k));
			MVS_HIP(hipGetLastError());
		}
		stream_wait(st, stream);
	}
	void search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, hipStream_t st) override {
		search_mapped(nq, d_x, k, d_D, d_I, params, nullptr, st);
	}
	bool named_stat(const char *name, int64_t *value) override {
		if (!strcmp(name, "sq_pair_block"))
			*value = sq_pair_block(d);
		else if (!strcmp(name, "sq_rows_per_workgroup"))
			*value = SQ_ROWS_PER_WG;
		else if (!strcmp(name, "sq_scan_launches"))
			*value = last_launches;
		else if (!strcmp(name, "sq_scan_rescans"))
			*value = last_rescans;
		else if (!strcmp(name, "sq_device_bytes"))
			*value = (int64_t)device_bytes();
		else
			return false;
		return true;
	}
	size_t device_bytes() const override {
		return (size_t)cap * pitch + lcodes.cap + lids.cap + (d_par ? (size_t)4 * d * sizeof(float) : 0);
	}

	// ------------------------------------------------------------------------------------------ images, placement
	// SQ8: codes [ntotal][d]; IVF: ArrayInvertedLists image, per list d-byte codes and ids in arrival order
	void to_host(HostIndex &out) override {
		use_device();
		MVS_HIP(hipStreamSynchronize(stream));
		build_lists();
		out.kind = kind;
		out.d = d;
		out.metric = metric;
		out.metric_arg = metric_arg;
		out.ntotal = ntotal;
		out.is_trained = is_trained;
		out.sq_trained.assign((size_t)2 * d, 0.f); // (an image without a range: zeros here, an empty vector in a file)
		out.sq_has_range = have_par;
		if (have_par)
			get_trained(out.sq_trained.data());
		std::vector<uint8_t> all((size_t)nsorted * d);
		if (nsorted > 0)
			MVS_HIP(hipMemcpy2D(all.data(), (size_t)d, list_codes(), (size_t)pitch, (size_t)d, (size_t)nsorted, hipMemcpyDeviceToHost));
		if (!ivf) {
			out.sq_codes.swap(all);
			return;
		}
		out.nlist = nlist;
		out.nprobe = nprobe;
		out.sub.reset(new HostIndex);
		quantizer->to_host(*out.sub);
		out.list_ids.assign((size_t)nlist, {});
		out.list_bytes.assign((size_t)nlist, {});
		for (int64_t l = 0; l < nlist; l++) {
			const int64_t b = list_off[(size_t)l], e = list_off[(size_t)l + 1];
			out.list_ids[(size_t)l].assign(sid_h.begin() + b, sid_h.begin() + e);
			out.list_bytes[(size_t)l].assign(all.begin() + b * d, all.begin() + e * d);
		}
	}
	// an empty index on its device <- range and codes of the image (the quantiser is loaded by the caller); IVF rows enter in list order,
	// which keeps the arrival order inside every list
	void load_image(const HostIndex &h) {
		const char *fn = "faiss::Index* faiss::read_index(...)", *file = "faiss/impl/index_read.cpp";
		if (h.sq_trained.size() != (size_t)2 * d)
			throw_faiss(fn, file, "SQ8 image: %zu trained values for d = %d", h.sq_trained.size(), d);
		int64_t n = 0;
		if (!ivf) {
			if ((int64_t)h.sq_codes.size() != h.ntotal * d)
				throw_faiss(fn, file, "Error: 'idxs->codes.size() == idxs->ntotal * idxs->code_size' failed");
			n = h.ntotal;
		} else {
			if ((int64_t)h.list_ids.size() != nlist || (int64_t)h.list_bytes.size() != nlist)
				throw_faiss(fn, file, "IVFSQ image: inverted lists do not match nlist = %lld", (long long)nlist);
			for (int64_t l = 0; l < nlist; l++) {
				if (h.list_bytes[(size_t)l].size() != h.list_ids[(size_t)l].size() * (size_t)d)
					throw_faiss(fn, file, "IVFSQ image: list %lld holds %zu code bytes for %zu ids", (long long)l, h.list_bytes[(size_t)l].size(),
					            h.list_ids[(size_t)l].size());
				n += (int64_t)h.list_ids[(size_t)l].size();
			}
		}
		if (n > (int64_t)0x7fffffff - 1024)
			throw_faiss("mvs::SQIndex::add", __FILE__, "a single-device index holds at most 2^31 rows");
		use_device();
		metric_arg = h.metric_arg;
		nprobe = h.nprobe;
		if (h.is_trained || h.sq_has_range)
			set_trained(h.sq_trained.data());
		cent_dirty = true;
		update_trained();
		grow(n);
		const uint8_t *src = h.sq_codes.data();
		std::vector<uint8_t> all;
		if (ivf) {
			all.resize((size_t)n * d);
			assign_h.clear();
			ids_h.clear();
			int64_t r = 0;
			for (int64_t l = 0; l < nlist; l++) {
				const auto &li = h.list_ids[(size_t)l];
				if (!li.empty())
					memcpy(&all[(size_t)r * d], h.list_bytes[(size_t)l].data(), li.size() * (size_t)d);
				for (size_t j = 0; j < li.size(); j++, r++) {
					assign_h.push_back((int32_t)l);
					ids_h.push_back(li[j]);
				}
			}
			src = all.data();
		}
		if (n > 0)
			MVS_HIP(hipMemcpy2D(d_codes, (size_t)pitch, src, (size_t)d, (size_t)d, (size_t)n, hipMemcpyHostToDevice));
		ntotal = n;
		dirty = true;
	}
	void to_device(int new_device) override {
		if (new_device == device)
			return;
		int ndev = 0;
		MVS_HIP(hipGetDeviceCount(&ndev));
		if (new_device < 0 || new_device >= ndev)
			throw_faiss("faiss::gpu::index_cpu_to_gpu", "faiss/gpu/GpuCloner.cpp", "Invalid GPU device %d", new_device);
		HostIndex img;
		to_host(img);
		use_device();
		MVS_HIP(hipStreamSynchronize(stream));
		pinned.drop_events();
		free_device();
		have_par = false;
		ws_hx.release();
		ws_hD.release();
		ws_hI.release();
		MVS_HIP(hipStreamDestroy(stream));
		stream = nullptr;
		if (quantizer)
			quantizer->to_device(new_device);
		MVS_HIP(hipSetDevice(new_device));
		MVS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
		device = new_device;
		ntotal = 0;
		load_image(img);
	}
	IndexBase *clone(int on_device) override {
		int ndev = 0;
		MVS_HIP(hipGetDeviceCount(&ndev));
		if (on_device < 0 || on_device >= ndev)
			throw_faiss("faiss::gpu::index_cpu_to_gpu", "faiss/gpu/GpuCloner.cpp", "Invalid GPU device %d", on_device);
		HostIndex img;
		to_host(img);
		IndexBase *c = sq_from_host(img, on_device);
		c->label_offset = label_offset;
		return c;
	}
};

SQIndex *as_sq(IndexBase *ix) {
	return ix && (ix->kind == MVS_KIND_SQ || ix->kind == MVS_KIND_IVFSQ) ? static_cast<SQIndex *>(ix) : nullptr;
}
SQIndex *as_ivfsq(IndexBase *ix) {
	return ix && ix->kind == MVS_KIND_IVFSQ ? static_cast<SQIndex *>(ix) : nullptr;
}

} // namespace

// "SQ8" | "IVF<n>,SQ8" (faiss/index_factory.cpp); nullptr if desc is neither an SQ string nor an IVF string whose codes are SQ
IndexBase *make_sq_index(int d, const std::string &desc, int metric) {
	const char *fn = "faiss::Index* faiss::index_factory(int, const char*, faiss::MetricType)";
	const char *sq = nullptr;
	long nlist = 0;
	if (desc.rfind("SQ", 0) == 0) {
		sq = desc.c_str();
	} else if (desc.rfind("IVF", 0) == 0) {
		char *end = nullptr;
		nlist = strtol(desc.c_str() + 3, &end, 10);
		if (end == desc.c_str() + 3 || nlist <= 0)
			return nullptr;
		const char *comma = strchr(end, ',');
		if (!comma || strncmp(comma + 1, "SQ", 2) != 0)
			return nullptr;
		if (comma != end) // "IVF<n>_HNSW<m>,SQ8": only the Flat coarse quantiser
			throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s (Flat coarse quantizer only)",
			            desc.c_str());
		sq = comma + 1;
	} else {
		return nullptr;
	}
	if (strcmp(sq, "SQ8") != 0) // SQ4, SQ6, SQfp16, SQbf16, SQ8_direct, ...
		throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s (8-bit uniform scalar quantizer only)",
		            desc.c_str());
	if (d > SQ_MAX_D)
		throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s at d = %d (at most %d dimensions)",
		            desc.c_str(), d, SQ_MAX_D);
	return new SQIndex(d, nlist, metric);
}
IndexBase *sq_from_host(const HostIndex &h, int device) {
	CtorDevice scope(device);
	const char *fn = "faiss::Index* faiss::read_index(...)", *file = "faiss/impl/index_read.cpp";
	const bool ivf = h.kind == MVS_KIND_IVFSQ;
	if (h.d <= 0 || h.d > SQ_MAX_D || (ivf && h.nlist <= 0))
		throw_faiss(fn, file, "SQ8 image with d = %d, nlist = %lld is not served on the MI355X path", h.d, (long long)h.nlist);
	if (ivf) {
		if (!h.sub || h.sub->kind != MVS_KIND_FLAT)
			throw_faiss(fn, file, "only a Flat coarse quantizer is implemented for IVFSQ on the MI355X path");
		if (h.sub->ntotal != 0 && (h.sub->ntotal != h.nlist || h.sub->d != h.d))
			throw_faiss(fn, file, "IVFSQ image: the quantizer holds %lld rows for nlist = %lld", (long long)h.sub->ntotal, (long long)h.nlist);
	}
	auto *p = new SQIndex(h.d, ivf ? h.nlist : 0, h.metric);
	try {
		if (ivf && h.sub->ntotal > 0)
			p->quantizer->add(h.sub->ntotal, h.sub->rows.data());
		p->load_image(h);
	} catch (...) {
		delete p;
		throw;
	}
	return p;
}
IndexBase *ivfsq_quantizer_of(IndexBase *ix) {
	SQIndex *p = as_ivfsq(ix);
	return p ? p->quantizer : nullptr;
}
int64_t ivfsq_nlist_of(IndexBase *ix) {
	SQIndex *p = as_ivfsq(ix);
	return p ? p->nlist : 0;
}
bool ivfsq_get_coarse(IndexBase *ix, float *out) {
	SQIndex *p = as_ivfsq(ix);
	if (p)
		p->get_coarse(out);
	return p != nullptr;
}
bool ivfsq_set_coarse(IndexBase *ix, const float *c) {
	SQIndex *p = as_ivfsq(ix);
	if (p)
		p->set_coarse(c);
	return p != nullptr;
}
bool sq_get_trained(IndexBase *ix, float *out) {
	SQIndex *p = as_sq(ix);
	if (p)
		p->get_trained(out);
	return p != nullptr || hnswsq_get_trained(ix, out);
}
bool sq_set_trained(IndexBase *ix, const float *t) {
	SQIndex *p = as_sq(ix);
	if (p)
		p->set_trained(t);
	return p != nullptr || hnswsq_set_trained(ix, t);
}
bool sq_get_codes(IndexBase *ix, int64_t row0, int64_t n, uint8_t *out) {
	if (ix->kind != MVS_KIND_SQ)
		return hnswsq_get_codes(ix, row0, n, out); // ("HNSW<M>,SQ8": vertex order)
	static_cast<SQIndex *>(ix)->get_codes(row0, n, out);
	return true;
}
int64_t ivfsq_list_size(IndexBase *ix, int64_t list_no) {
	SQIndex *p = as_ivfsq(ix);
	if (!p)
		throw_faiss("mvs_index_ivfsq_list_size", __FILE__, "not an IVFSQ index");
	return p->list_size(list_no);
}
void ivfsq_get_list(IndexBase *ix, int64_t list_no, int64_t *ids, uint8_t *codes) {
	SQIndex *p = as_ivfsq(ix);
	if (!p)
		throw_faiss("mvs_index_ivfsq_get_list", __FILE__, "not an IVFSQ index");
	p->get_list(list_no, ids, codes);
}

} // namespace mvs
