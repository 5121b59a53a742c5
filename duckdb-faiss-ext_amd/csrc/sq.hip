// csrc/sq.hip -- "SQ8" (faiss::IndexScalarQuantizer) and "IVF<n>,SQ8" (faiss::IndexIVFScalarQuantizer, an IndexIVF: the dynamic_cast of
// src/faiss_extension.cpp:675 sets nprobe on it): one byte per component, a per-dimension range learnt from min / max.
//
// Contract (include/mi355_faiss.h "8-bit scalar-quantised indexes"):
//   train   vmin[k], vdiff[k] = max - min of component k over the training rows (IVF: over their residuals x - c against the k = 1
//           centroid; the coarse centroids are what IVF<n>,Flat of the same metric learns); s[k] = vdiff[k] / 255, a[k] = vmin[k] + 0.5 s[k]
//   add     code[k] = (int)(255 * clamp((y - vmin[k]) / vdiff[k], 0, 1)), 0 where vdiff[k] == 0; y = x[k] or the residual
//   search  dec(c, k) = a[k] + (float)c * s[k]; L2: acc = fmaf(t, t, acc), t = v[k] - dec, v = x - c (IVF) or x; inner product:
//           acc = fmaf(x[k], dec, acc), IVF: + the chain <x, c>; the k best in the PURE order: distance, then probe rank, then position
//           -- among the values the ADMISSION RULE of csrc/pq_kernels.h lets in: no NaN, nothing that is not strictly better than FLT_MAX
//           (L2) / -FLT_MAX (inner product)
//
// EVERY operation above is one IEEE f32 operation rounded on its own.  Device code is compiled with floating-point contraction on, and
// __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn are plain operators that inline INTO that mode: a[k] + c * s[k] written with them still
// becomes one fma.  The whole translation unit is therefore compiled with contraction off (the pragma below, which the compiler's default
// mode for device code honours), the rounded operations are the sq_* helpers under it, and the chains are explicit fmaf calls.
//
// SQ8 is the degenerate case of the IVF machinery: ONE list that holds every row in arrival order (the arrival-order store itself: no
// second copy), no centroid (v = x, no base), probe rank 0 for every query; (distance, rank, position) is then (distance, row).
//
// The host driver -- coarse side, code store, list view, units of (rank span, position window), selection, images -- is CodedListsIndex
// (csrc/coded_lists.hip); a unit of ONE rank is walked in tripling windows here.  Here: the range, the encoder and the scan.
//
// Kernels
//   sq8_minmax_kernel / sq8_minmax_fold_kernel   (csrc/sq8_kernels.h, shared with csrc/hnsw.hip's "HNSW<M>,SQ8") two-stage min / max per
//                             component over (the residuals of) a batch of training rows
//   sq8_derive_kernel         (csrc/sq8_kernels.h) vdiff, s, a from the range
//   sq8_encode_kernel         (csrc/sq8_kernels.h) residual + code, one lane per component
//   sq8_scan_kernel<Q, L2>    the hot path: a workgroup takes (<= Q pairs of one list, <= R positions of it).  The pairs' vectors sit in LDS
//                             interleaved [k][Q]: one broadcast 16-byte read hands a lane four pairs' values of component k.  A lane owns a
//                             row; the codes of 1024 rows travel through LDS in chunks of 32 components (coalesced 16-byte loads, rows at a
//                             pitch of 48 bytes -- an odd number of 16-byte words -- so that a lane's own 16-byte reads do not collide); one
//                             conversion and the two-operation decode per component serve all Q pairs, then one subtraction and one fmaf
//                             (L2) or one fmaf (inner product) per pair.  A value strictly below its query's bound goes to the query's
//                             bucket as (order key, ordinal)
#include "coded_lists.h"
#include "pq_kernels.h"
#include "sq8_kernels.h"

#include <algorithm>
#include <cstring>

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
typedef CodedScan SqScan; // par: [4][d] vmin | vdiff | a | s

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
	float *s_thr = reinterpret_cast<float *>(s_ord + SQ_MAX_Q); // the bounds as values (pq_bound_value)
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
		s_q[tid] = q, s_ord[tid] = ord, s_thr[tid] = pq_bound_value(th, L2 ? 0 : 1), s_base[tid] = acc;
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
			if (pq_beats(v, s_thr[s], pq_sign_mask(L2 ? 0 : 1))) {
				const unsigned key = pq_key(v, L2 ? 0 : 1);
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

// ---------------------------------------------------------------------------------------------- index
class SQIndex : public CodedListsIndex {
public:
	const bool ivf;

	SQIndex(int d_, int64_t nlist_, int metric_)
	    : CodedListsIndex(nlist_ > 0 ? MVS_KIND_IVFSQ : MVS_KIND_SQ, d_, metric_, nlist_, d_, (size_t)4 * d_, true,
	                      {"mvs::SQIndex", __FILE__, "SQ8", "IVFSQ",
	                       nlist_ > 0 ? "virtual void faiss::IndexIVFScalarQuantizer::add_core(...)" : "virtual void faiss::IndexFlatCodes::add(...)",
	                       nlist_ > 0 ? "faiss/IndexScalarQuantizer.cpp" : "faiss/IndexFlatCodes.cpp", "sq", &HostIndex::sq_codes}),
	      ivf(nlist_ > 0) {
	}

	// ------------------------------------------------------------------------------------------ train
	void check_empty_for_training() const override {
		if (ntotal > 0)
			throw_faiss("mvs::SQIndex::train", __FILE__, "the index already holds %lld rows encoded with its range%s: "
			            "training again is only possible while it is empty", (long long)ntotal, ivf ? " and centroids" : "");
	}
	void derive(bool from_range) { // (on `stream`)
		hipLaunchKernelGGL(sq8_derive_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, stream, d_par(), d, from_range ? 1 : 0);
		MVS_HIP(hipGetLastError());
		MVS_HIP(hipStreamSynchronize(stream));
		have_par = true;
		update_trained();
	}
	void set_trained(const float *t) { // [2][d] vmin | vdiff
		use_device();
		check_empty_for_training();
		ensure_par();
		MVS_HIP(hipMemcpyAsync(d_par(), t, (size_t)2 * d * sizeof(float), hipMemcpyHostToDevice, stream));
		derive(false);
	}
	void get_trained(float *out) {
		use_device();
		if (!have_par)
			throw_faiss("mvs::SQIndex::get_trained", __FILE__, "the index has no trained range yet");
		MVS_HIP(hipStreamSynchronize(stream));
		MVS_HIP(hipMemcpy(out, d_par(), (size_t)2 * d * sizeof(float), hipMemcpyDeviceToHost));
	}
	void train(int64_t n, const float *x) override {
		use_device();
		check_empty_for_training();
		n = std::max<int64_t>(n, 0);
		CtorDevice scope(device);
		if (ivf)
			train_coarse(n, x);
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
		ws_kind.reserve((size_t)chunks_max * 2 * d * sizeof(float));
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
			                   (const long long *)d_lab, d_cent, (long long)nlist, (float *)ws_kind.p);
			hipLaunchKernelGGL(sq8_minmax_fold_kernel, dim3(gk), dim3(256), 0, stream, (const float *)ws_kind.p, chunks, d, d_par(), i0 == 0 ? 1 : 0);
			MVS_HIP(hipGetLastError());
			MVS_HIP(hipStreamSynchronize(stream)); // (ws_add is filled again)
		}
		derive(true);
	}

	// ------------------------------------------------------------------------------------------ add, search: what CodedListsIndex asks for
	void encode_block(int64_t nb, const float *d_x, const int64_t *d_lab, int64_t first_row) override {
		const long long tot = nb * d;
		hipLaunchKernelGGL(sq8_encode_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, d_x, (long long)nb, d, (const long long *)d_lab,
		                   centroids_dev(), (long long)nlist, (const float *)d_par(), store.codes(), store.pitch, (long long)first_row);
	}
	int pair_block() const override {
		return sq_pair_block(d);
	}
	void launch_scan_kernel(const CodedScan &a, dim3 grid, int64_t nqc, double rows) override {
		const int Q = pair_block();
		const size_t lds = sq_scan_lds(d, Q);
#define SQ_LAUNCH_SCAN(QQ, LL)                                                                                                                      \
	do {                                                                                                                                            \
		ensure_dynamic_lds((const void *)sq8_scan_kernel<QQ, LL>, lds);                                                                             \
		hipLaunchKernelGGL((sq8_scan_kernel<QQ, LL>), grid, dim3(SQ_THREADS), lds, stream, a);                                                      \
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
		set_kinfo("sq8_scan_kernel", (double)nqc * rows * d * (l2 ? 3.0 : 2.0), (double)nqc * rows * d / Q, (int)(grid.x * grid.y), SQ_THREADS, (int)lds,
		          (int)grid.y);
	}
	void get_codes(int64_t row0, int64_t n, uint8_t *out) { // SQ8: rows of the arrival-order store
		use_device();
		if (row0 < 0 || n < 0 || row0 + n > ntotal)
			throw_faiss("mvs::SQIndex::get_codes", __FILE__, "rows [%lld, %lld) are outside the index (ntotal %lld)", (long long)row0,
			            (long long)(row0 + n), (long long)ntotal);
		MVS_HIP(hipStreamSynchronize(stream));
		if (n > 0)
			MVS_HIP(hipMemcpy2D(out, (size_t)d, store.codes() + (size_t)row0 * store.pitch, (size_t)store.pitch, (size_t)d, (size_t)n, hipMemcpyDeviceToHost));
	}
	bool named_stat(const char *name, int64_t *value) override {
		if (strcmp(name, "sq_device_bytes") != 0)
			return CodedListsIndex::named_stat(name, value);
		*value = (int64_t)device_bytes();
		return true;
	}

	// ------------------------------------------------------------------------------------------ images
	void check_image(const HostIndex &h) const override {
		const char *fn = "faiss::Index* faiss::read_index(...)", *file = "faiss/impl/index_read.cpp";
		if (h.sq_trained.size() != (size_t)2 * d)
			throw_faiss(fn, file, "SQ8 image: %zu trained values for d = %d", h.sq_trained.size(), d);
		if (!ivf && (int64_t)h.sq_codes.size() != h.ntotal * d)
			throw_faiss(fn, file, "Error: 'idxs->codes.size() == idxs->ntotal * idxs->code_size' failed");
		if (ivf && ((int64_t)h.list_ids.size() != nlist || (int64_t)h.list_bytes.size() != nlist))
			throw_faiss(fn, file, "IVFSQ image: inverted lists do not match nlist = %lld", (long long)nlist);
	}
	void params_to_host(HostIndex &out) override {
		out.sq_trained.assign((size_t)2 * d, 0.f); // (an image without a range: zeros here, an empty vector in a file)
		out.sq_has_range = have_par;
		if (have_par)
			get_trained(out.sq_trained.data());
	}
	void params_from_host(const HostIndex &h) override {
		if (h.is_trained || h.sq_has_range)
			set_trained(h.sq_trained.data());
	}
};

SQIndex *as_sq(IndexBase *ix) {
	return ix && (ix->kind == MVS_KIND_SQ || ix->kind == MVS_KIND_IVFSQ) ? static_cast<SQIndex *>(ix) : nullptr;
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
			p->coarse.quantizer->add(h.sub->ntotal, h.sub->rows.data());
		p->load_image(h);
	} catch (...) {
		delete p;
		throw;
	}
	return p;
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

} // namespace mvs
