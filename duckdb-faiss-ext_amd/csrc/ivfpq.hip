// csrc/ivfpq.hip -- "IVF<n>,PQ<M>" (faiss::IndexIVFPQ, an IndexIVF: the dynamic_cast of src/faiss_extension.cpp:675 sets nprobe on it):
// inverted lists of product-quantised RESIDUALS, 8 bits per code, by_residual under both metrics.
//
// Contract (include/mi355_faiss.h "inverted lists of product-quantised residuals"):
//   train   coarse centroids = what IVF<n>,Flat of the same metric learns from x; every training row's residual against its k = 1
//           centroid; codebook m = what IVF256,Flat (L2) learns from columns [m dsub, (m+1) dsub) of all residuals in input order
//   add     list = the quantiser's k = 1 label; code = pq_encode_kernel's rule on x - c; rows appended to their list in arrival order
//   search  per (query, probed list): v = x - c (L2) or x (inner product); T[m][j] = the L2 / ip chain of v's sub-vector m against
//           codebook entry j; dis = ((T[0][c0] + T[1][c1]) + ...) -- under inner product started from base = the ip chain <x, c>; the
//           k best in the PURE order: distance, then probe rank, then position in the list -- among the values the ADMISSION RULE of
//           csrc/pq_kernels.h lets in: no NaN, nothing that is not strictly better than FLT_MAX (L2) / -FLT_MAX (inner product)
//
// The host driver -- coarse side, code store, list view, units of (rank span, position window), selection, images -- is CodedListsIndex
// (csrc/coded_lists.hip).  Here: the codebooks, the encoder and the scan.
//
// Kernels
//   ivfpq_residual_kernel     x - centroid[label], one f32 subtraction per component
//   pq_encode_kernel          (csrc/pq_kernels.h) the residuals' codes
//   ivfpq_scan_kernel<W>      the hot path: a workgroup takes (<= Q pairs of one list, <= R rows of it), BUILDS the pairs' tables in LDS
//                             in pq.hip's interleaved layouts -- the codebooks streamed one sub-space at a time --, then walks the rows'
//                             code bytes as pq_scan_kernel does; a sum strictly below its query's bound goes to the query's bucket as
//                             (order key, ordinal)
#include "coded_lists.h"
#include "pq_kernels.h"

#include <algorithm>
#include <cstring>

namespace mvs {

namespace {

constexpr int IVFPQ_ROWS_PER_WG = PQ_ROWS_PER_WG; // rows of a list one scan workgroup walks = bucket entries (pq_select_kernel's pitch)
constexpr int IVFPQ_VSTAGE_FLOATS = 4096;         // LDS floats for the pairs' v vectors (Q d beyond that: v is formed from global memory)
constexpr int IVFPQ_MAX_Q = 32;                   // pq_width * pq_groups at most
constexpr int IVFPQ_PAIRS_PER_THREAD = 8;               // table build: chains a lane runs at once (one codebook value, 8 pairs)

// ---------------------------------------------------------------------------------------------- residuals, list view
__global__ __launch_bounds__(256) void ivfpq_residual_kernel(const float *__restrict__ x, long long n, int d, const long long *__restrict__ label,
                                                             const float *__restrict__ cent, long long nlist, float *__restrict__ out) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n * d)
		return;
	const long long r = i / d;
	const int k = (int)(i - r * d);
	const long long l = label[r];
	out[i] = l >= 0 && l < nlist ? x[i] - cent[l * d + k] : x[i]; // (a row without a list is stored nowhere: its code is never read)
}

// ---------------------------------------------------------------------------------------------- scan
struct IvfpqScan : CodedScan { // par: the codebooks [M][256][dsub]
	int M, dsub, G, is_l2;
};

// workgroup blockIdx.x = one pair group (<= Q pairs of one list), blockIdx.y = the segment of R positions of the window
template <int W>
__global__ __launch_bounds__(PQ_SCAN_THREADS) void ivfpq_scan_kernel(const IvfpqScan a) {
	extern __shared__ __attribute__((aligned(16))) float4 ivfpq_lds[];
	typedef typename PqEntry<W>::type entry_t;
	const int tid = threadIdx.x, Q = W * a.G, g = blockIdx.x;
	if (g >= a.goff[a.nlist])
		return;
	int lo = 0, hi = a.nlist; // goff[lo] <= g < goff[hi]: the list with goff[l] <= g < goff[l + 1]
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
	const long long s0 = a.p0 + (long long)blockIdx.y * IVFPQ_ROWS_PER_WG;
	if (s0 >= w1)
		return; // (uniform over the workgroup: no barrier has been reached)
	const long long s1 = s0 + IVFPQ_ROWS_PER_WG < w1 ? s0 + IVFPQ_ROWS_PER_WG : w1;
	const int pj = a.poff[l] + (g - a.goff[l]) * Q;
	const int npg = a.poff[l + 1] - pj < Q ? a.poff[l + 1] - pj : Q; // pairs of this group, >= 1
	const int d = a.d, M = a.M, dsub = a.dsub;
	// LDS: tables [G][M][256][W] | v [Q][d] (if it fits) | base [32] | query [32] | ordinal base [32]
	float *T = reinterpret_cast<float *>(ivfpq_lds);
	float *vst = T + (size_t)Q * M * PQ_KSUB;
	float *s_base = vst + IVFPQ_VSTAGE_FLOATS;
	int *s_q = reinterpret_cast<int *>(s_base + IVFPQ_MAX_Q);
	unsigned *s_ord = reinterpret_cast<unsigned *>(s_q + IVFPQ_MAX_Q);
	const bool v_in_lds = Q * d <= IVFPQ_VSTAGE_FLOATS;
	const float *cl = a.cent + (size_t)l * d;
	if (tid < npg) {
		const int2 p = a.pairs[pj + tid];
		s_q[tid] = p.x;
		s_ord[tid] = a.pref[(size_t)p.x * (a.np + 1) + p.y];
		float acc = 0.f;
		if (!a.is_l2) { // base = the ip chain <x, c>, k ascending
			const float *xv = a.xq + (size_t)p.x * d;
			for (int k = 0; k < d; ++k)
				acc = fmaf(xv[k], cl[k], acc);
		}
		s_base[tid] = acc;
	}
	__syncthreads();
	if (v_in_lds) {
		for (int i = tid; i < npg * d; i += PQ_SCAN_THREADS) {
			const int s = i / d, k = i - s * d;
			const float xv = a.xq[(size_t)s_q[s] * d + k];
			vst[i] = a.is_l2 ? xv - cl[k] : xv;
		}
		__syncthreads();
	}
	{ // tables: lane j = tid & 255 takes codebook entry j; the workgroup's quarter tid / 256 takes the sub-spaces m = quarter, quarter + 4, ...
		// -- every codebook value is loaded once per workgroup and block of 8 pairs (Q <= 8: once)
		const int j = tid & 255;
		for (int m = tid >> 8; m < M; m += PQ_SCAN_THREADS / PQ_KSUB) {
			const float *cbj = a.par + ((size_t)m * PQ_KSUB + j) * dsub;
			for (int s0p = 0; s0p < npg; s0p += IVFPQ_PAIRS_PER_THREAD) {
				float acc[IVFPQ_PAIRS_PER_THREAD];
#pragma unroll
				for (int i = 0; i < IVFPQ_PAIRS_PER_THREAD; ++i)
					acc[i] = 0.f;
				for (int k = 0; k < dsub; ++k) {
					const float c = cbj[k];
					const int col = m * dsub + k;
#pragma unroll
					for (int i = 0; i < IVFPQ_PAIRS_PER_THREAD; ++i) {
						const int s = s0p + i;
						if (s < npg) {
							float v;
							if (v_in_lds) {
								v = vst[s * d + col];
							} else {
								const float xv = a.xq[(size_t)s_q[s] * d + col];
								v = a.is_l2 ? xv - cl[col] : xv;
							}
							if (a.is_l2) {
								const float t = v - c;
								acc[i] = fmaf(t, t, acc[i]);
							} else {
								acc[i] = fmaf(v, c, acc[i]);
							}
						}
					}
				}
#pragma unroll
				for (int i = 0; i < IVFPQ_PAIRS_PER_THREAD; ++i) {
					const int s = s0p + i;
					if (s < npg)
						T[(((size_t)(s / W) * M + m) * PQ_KSUB + j) * W + (s % W)] = acc[i];
				}
			}
		}
	}
	__syncthreads();
	const int descending = a.is_l2 ? 0 : 1;
	const unsigned smask = pq_sign_mask(descending);
	for (int gq = 0; gq < a.G; ++gq) {
		const int sg0 = gq * W;
		if (sg0 >= npg)
			break;
		unsigned ob[W];
		int qq[W];
		float b0[W], th[W]; // th: the bounds as values (pq_bound_value)
#pragma unroll
		for (int w = 0; w < W; ++w) {
			const bool valid = sg0 + w < npg;
			qq[w] = valid ? s_q[sg0 + w] : 0;
			th[w] = pq_bound_value(valid ? a.thr[qq[w]] : 0u, descending); // (0: no key is below it -- a slot without a pair admits nothing)
			ob[w] = valid ? s_ord[sg0 + w] : 0u;
			b0[w] = valid ? s_base[sg0 + w] : 0.f;
		}
		const entry_t *Tg = reinterpret_cast<const entry_t *>(T) + (size_t)gq * M * PQ_KSUB;
		for (long long pos = s0 + tid; pos < s1; pos += PQ_SCAN_THREADS) {
			const long long row = lb + pos;
			if (a.sel.kind != MVS_SEL_NONE) {
				const long long id = a.lids[row];
				if (!pq_sel_member(a.sel, a.idmap ? a.idmap[id] : id))
					continue;
			}
			const uint4 *cr = reinterpret_cast<const uint4 *>(a.codes + row * a.pitch);
			float acc[W];
#pragma unroll
			for (int w = 0; w < W; ++w)
				acc[w] = b0[w]; // (L2: 0 + T is T bit for bit, no entry is -0; inner product: the chain starts from base)
			for (int c = 0; c < M; c += 16) {
				const uint4 cw = cr[c >> 4];
				const unsigned wd[4] = {cw.x, cw.y, cw.z, cw.w};
				if (c + 16 <= M) {
#pragma unroll
					for (int b = 0; b < 16; ++b) {
						const unsigned code = (wd[b >> 2] >> ((b & 3) * 8)) & 255u;
						PqEntry<W>::add(acc, Tg[(c + b) * PQ_KSUB + code]);
					}
				} else {
#pragma unroll
					for (int b = 0; b < 16; ++b)
						if (c + b < M) {
							const unsigned code = (wd[b >> 2] >> ((b & 3) * 8)) & 255u;
							PqEntry<W>::add(acc, Tg[(c + b) * PQ_KSUB + code]);
						}
				}
			}
#pragma unroll
			for (int w = 0; w < W; ++w) {
				if (pq_beats(acc[w], th[w], smask)) {
					const unsigned key = pq_key(acc[w], descending);
					const unsigned at = atomicAdd(&a.cnt[qq[w]], 1u);
					if (at < (unsigned)IVFPQ_ROWS_PER_WG)
						a.bucket[(size_t)qq[w] * IVFPQ_ROWS_PER_WG + at] = ((unsigned long long)key << 32) | (unsigned long long)(ob[w] + (unsigned)pos);
					else
						*a.overflow = 1;
				}
			}
		}
	}
}

// ---------------------------------------------------------------------------------------------- index
class IVFPQIndex : public CodedListsIndex {
public:
	const int M, dsub;

	IVFPQIndex(int d_, int64_t nlist_, int M_, int metric_)
	    : CodedListsIndex(MVS_KIND_IVFPQ, d_, metric_, nlist_, M_, (size_t)M_ * PQ_KSUB * (d_ / M_), false,
	                      {"mvs::IVFPQIndex", __FILE__, "IVFPQ", "IVFPQ", "virtual void faiss::IndexIVFPQ::add_core(...)", "faiss/IndexIVFPQ.cpp", "ivfpq",
	                       nullptr}),
	      M(M_), dsub(d_ / M_) {
	}

	// ------------------------------------------------------------------------------------------ train
	void check_empty_for_training() const override {
		if (ntotal > 0)
			throw_faiss("mvs::IVFPQIndex::train", __FILE__, "the index already holds %lld rows encoded with its centroids and codebooks: "
			            "training again is only possible while it is empty", (long long)ntotal);
	}
	void set_codebooks(const float *c) {
		use_device();
		check_empty_for_training();
		ensure_par();
		MVS_HIP(hipMemcpyAsync(d_par(), c, par_floats * sizeof(float), hipMemcpyHostToDevice, stream));
		MVS_HIP(hipStreamSynchronize(stream));
		have_par = true;
		update_trained();
	}
	void get_codebooks(float *out) {
		use_device();
		if (!d_par())
			throw_faiss("mvs::IVFPQIndex::get_centroids", __FILE__, "the index has no codebooks yet");
		MVS_HIP(hipStreamSynchronize(stream));
		MVS_HIP(hipMemcpy(out, d_par(), par_floats * sizeof(float), hipMemcpyDeviceToHost));
	}
	void residuals_device(int64_t n, const float *d_x, const int64_t *d_lab, float *d_out) {
		const long long tot = n * d;
		hipLaunchKernelGGL(ivfpq_residual_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, d_x, (long long)n, d, (const long long *)d_lab,
		                   centroids_dev(), (long long)nlist, d_out);
		MVS_HIP(hipGetLastError());
	}
	void train(int64_t n, const float *x) override {
		use_device();
		check_empty_for_training();
		n = std::max<int64_t>(n, 0);
		CtorDevice scope(device);
		train_coarse(n, x); // 1. the coarse centroids
		// 2. every training row's residual against its k = 1 centroid, in input order
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
			residuals_device(nb, (const float *)ws_add.p, d_lab, (float *)ws_kind.p);
			MVS_HIP(hipMemcpyAsync(&res[(size_t)i0 * d], ws_kind.p, (size_t)nb * d * sizeof(float), hipMemcpyDeviceToHost, stream));
			MVS_HIP(hipStreamSynchronize(stream));
		}
		// 3. codebook m: 256 L2 clusters of the residuals' columns [m dsub, (m+1) dsub) -- also under inner product
		std::vector<float> cent(par_floats), cols((size_t)n * dsub);
		for (int m = 0; m < M; ++m) {
			for (int64_t i = 0; i < n; ++i)
				memcpy(&cols[(size_t)i * dsub], &res[(size_t)i * d + (size_t)m * dsub], (size_t)dsub * sizeof(float));
			FlatIndex assigner(dsub, METRIC_L2);
			assigner.adopt_tuning(tune_);
			// 10 iterations are this project's contract (include/mi355_faiss.h, tests/pq_reference.py); FAISS's ProductQuantizer::train runs 25
			kmeans_train({PQ_KSUB, 10, false}, n, cols.data(), assigner);
			assigner.copy_rows_to_host(&cent[(size_t)m * PQ_KSUB * dsub]);
		}
		set_codebooks(cent.data());
	}

	// ------------------------------------------------------------------------------------------ add, search: what CodedListsIndex asks for
	void encode_block(int64_t nb, const float *d_x, const int64_t *d_lab, int64_t first_row) override {
		ws_kind.reserve((size_t)nb * d * sizeof(float)); // (the first block of an add is its largest)
		residuals_device(nb, d_x, d_lab, (float *)ws_kind.p);
		const bool in_lds = dsub <= PQ_ENCODE_LDS_DSUB;
		const size_t lds = in_lds ? (size_t)2 * PQ_KSUB * dsub * sizeof(float) : 0;
		if (lds > (48u << 10))
			ensure_dynamic_lds((const void *)pq_encode_kernel, lds);
		hipLaunchKernelGGL(pq_encode_kernel, dim3((unsigned)((nb + 255) / 256), (unsigned)M), dim3(256), lds, stream, (const float *)ws_kind.p,
		                   (long long)nb, d, dsub, (const float *)d_par(), store.codes(), store.pitch, (long long)first_row, in_lds ? 1 : 0);
	}
	int pair_block() const override {
		return pq_width(M) * pq_groups(M);
	}
	void launch_scan_kernel(const CodedScan &c, dim3 grid, int64_t nqc, double rows) override {
		const int W = pq_width(M), Q = pair_block();
		const size_t lds = (size_t)Q * M * PQ_KSUB * sizeof(float) + (size_t)IVFPQ_VSTAGE_FLOATS * sizeof(float) + (size_t)3 * IVFPQ_MAX_Q * sizeof(float);
		IvfpqScan a;
		static_cast<CodedScan &>(a) = c;
		a.M = M, a.dsub = dsub, a.G = pq_groups(M), a.is_l2 = metric == METRIC_L2 ? 1 : 0;
#define IVFPQ_LAUNCH_SCAN(WW)                                                                                                                       \
	do {                                                                                                                                            \
		ensure_dynamic_lds((const void *)ivfpq_scan_kernel<WW>, lds);                                                                               \
		hipLaunchKernelGGL(ivfpq_scan_kernel<WW>, grid, dim3(PQ_SCAN_THREADS), lds, stream, a);                                                     \
	} while (0)
		if (W == 4)
			IVFPQ_LAUNCH_SCAN(4);
		else if (W == 2)
			IVFPQ_LAUNCH_SCAN(2);
		else
			IVFPQ_LAUNCH_SCAN(1);
#undef IVFPQ_LAUNCH_SCAN
		set_kinfo("ivfpq_scan_kernel", (double)nqc * rows * M, (double)nqc * rows * M / Q, (int)(grid.x * grid.y), PQ_SCAN_THREADS, (int)lds, (int)grid.y);
	}

	// ------------------------------------------------------------------------------------------ images
	void check_image(const HostIndex &h) const override {
		if ((int64_t)h.list_ids.size() != nlist || (int64_t)h.list_bytes.size() != nlist || h.pq_centroids.size() != par_floats)
			throw_faiss("faiss::Index* faiss::read_index(...)", "faiss/impl/index_read.cpp", "IVFPQ image: inverted lists or codebooks do not match "
			            "nlist = %lld, d = %d, M = %d", (long long)nlist, d, M);
	}
	void params_to_host(HostIndex &out) override {
		out.pq_M = M;
		out.pq_centroids.assign(par_floats, 0.f); // (FAISS allocates the codebooks with the ProductQuantizer: an image without them holds zeros)
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

IVFPQIndex *as_ivfpq(IndexBase *ix) {
	return ix && ix->kind == MVS_KIND_IVFPQ ? static_cast<IVFPQIndex *>(ix) : nullptr;
}

} // namespace

// "IVF<n>,PQ<M>" | "IVF<n>,PQ<M>x8" (faiss/index_factory.cpp); nullptr if desc is not an IVF string whose codes are PQ
IndexBase *make_ivfpq_index(int d, const std::string &desc, int metric) {
	if (desc.rfind("IVF", 0) != 0)
		return nullptr;
	char *end = nullptr;
	const long nlist = strtol(desc.c_str() + 3, &end, 10);
	if (end == desc.c_str() + 3 || nlist <= 0)
		return nullptr;
	const char *comma = strchr(end, ',');
	if (!comma || strncmp(comma + 1, "PQ", 2) != 0)
		return nullptr;
	const char *fn = "faiss::Index* faiss::index_factory(int, const char*, faiss::MetricType)";
	if (comma != end) // "IVF<n>_HNSW<m>,PQ<M>": only the Flat coarse quantiser
		throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s (Flat coarse quantizer only)",
		            desc.c_str());
	const char *pq = comma + 3;
	char *mend = nullptr;
	const long M = strtol(pq, &mend, 10);
	if (mend == pq || M <= 0)
		return nullptr;
	if (*mend) { // "x<nbits>": 8 only; anything else (PQ<M>np, PQ<M>x<b>fs, ...) is a variant this path does not have
		char *end2 = nullptr;
		const long nbits = *mend == 'x' ? strtol(mend + 1, &end2, 10) : 0;
		if (*mend != 'x' || end2 == mend + 1 || *end2 || nbits != 8)
			throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s (8 bits per code only)",
			            desc.c_str());
	}
	if (M > PQ_MAX_M)
		throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s (at most %d subquantizers)",
		            desc.c_str(), PQ_MAX_M);
	if (d % M != 0)
		throw_faiss("faiss::ProductQuantizer::set_derived_values()", "faiss/impl/ProductQuantizer.cpp",
		            "Error: 'd %% M == 0' failed: The dimension of the vector (d) should be a multiple of the number of subquantizers (M)");
	return new IVFPQIndex(d, nlist, (int)M, metric);
}
IndexBase *ivfpq_from_host(const HostIndex &h, int device) {
	CtorDevice scope(device);
	if (!h.sub || h.sub->kind != MVS_KIND_FLAT)
		throw_faiss("faiss::Index* faiss::read_index(...)", "faiss/impl/index_read.cpp",
		            "only a Flat coarse quantizer is implemented for IVFPQ on the MI355X path");
	if (h.nlist <= 0 || h.pq_M <= 0 || h.pq_M > PQ_MAX_M || h.d % h.pq_M != 0)
		throw_faiss("faiss::Index* faiss::read_index(...)", "faiss/impl/index_read.cpp",
		            "IVFPQ image with nlist = %lld, M = %d at d = %d is not served on the MI355X path", (long long)h.nlist, h.pq_M, h.d);
	if (h.sub->ntotal != 0 && (h.sub->ntotal != h.nlist || h.sub->d != h.d))
		throw_faiss("faiss::Index* faiss::read_index(...)", "faiss/impl/index_read.cpp", "IVFPQ image: the quantizer holds %lld rows for nlist = %lld",
		            (long long)h.sub->ntotal, (long long)h.nlist);
	auto *p = new IVFPQIndex(h.d, h.nlist, h.pq_M, h.metric);
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
bool ivfpq_info(const IndexBase *ix, int *M, int *nbits) {
	if (ix->kind != MVS_KIND_IVFPQ)
		return false;
	if (M)
		*M = static_cast<const IVFPQIndex *>(ix)->M;
	if (nbits)
		*nbits = 8;
	return true;
}
bool ivfpq_get_codebooks(IndexBase *ix, float *out) {
	IVFPQIndex *p = as_ivfpq(ix);
	if (p)
		p->get_codebooks(out);
	return p != nullptr;
}
bool ivfpq_set_codebooks(IndexBase *ix, const float *c) {
	IVFPQIndex *p = as_ivfpq(ix);
	if (p)
		p->set_codebooks(c);
	return p != nullptr;
}

} // namespace mvs
