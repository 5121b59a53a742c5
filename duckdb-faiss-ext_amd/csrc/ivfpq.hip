// csrc/ivfpq.hip -- "IVF<n>,PQ<M>" (faiss::IndexIVFPQ, an IndexIVF: the dynamic_cast of src/faiss_extension.cpp:675 sets nprobe on it):
// inverted lists of product-quantised RESIDUALS, 8 bits per code, by_residual under both metrics.
//
// Contract (include/mi355_faiss.h "inverted lists of product-quantised residuals"):
//   train   coarse centroids = what IVF<n>,Flat of the same metric learns from x; every training row's residual against its k = 1
//           centroid; codebook m = what IVF256,Flat (L2) learns from columns [m dsub, (m+1) dsub) of all residuals in input order
//   add     list = the quantiser's k = 1 label; code = pq_encode_kernel's rule on x - c; rows appended to their list in arrival order
//   search  per (query, probed list): v = x - c (L2) or x (inner product); T[m][j] = the L2 / ip chain of v's sub-vector m against
//           codebook entry j; dis = ((T[0][c0] + T[1][c1]) + ...) -- under inner product started from base = the ip chain <x, c>; the
//           k best in the PURE order: distance, then probe rank, then position in the list
//
// Kernels
//   ivfpq_residual_kernel     x - centroid[label], one f32 subtraction per component
//   (ivfpq_gather_codes / prefix / count / offsets / scatter_kernel live in csrc/ivf_units.h: csrc/sq.hip runs them too)
//   ivfpq_prefix_kernel       per query the exclusive prefix of its probed lists' sizes in rank order: the base of its ORDINALS
//   ivfpq_count / offsets / scatter_kernel   the (query, rank) pairs of one unit grouped by list: a counting sort on the device
//   ivfpq_scan_kernel<W>      the hot path: a workgroup takes (<= Q pairs of one list, <= R rows of it), BUILDS the pairs' tables in LDS
//                             in pq.hip's interleaved layouts -- the codebooks streamed one sub-space at a time --, then walks the rows'
//                             code bytes as pq_scan_kernel does; a sum strictly below its query's bound goes to the query's bucket as
//                             (order key, ordinal)
//   pq_select_kernel          (csrc/pq_kernels.h) list + bucket sorted, the k best stay, the k-th key becomes the bound
//   ivfpq_emit_kernel         ordinal -> (rank, position) -> stored id (IDMap: id_map[id]), -1 / FLT_MAX padded
//
// Selection.  pq.hip's range scheme over PROBE RANKS: [0, 1), [1, 3), [3, 9), ...  An entry's ordinal = rows of the lower ranks' lists +
// its position, so later units only bring larger ordinals than every list member: an entry tied at the bound never reaches the
// stream and the pure order comes out by construction.  A unit is (rank span, position window); a bucket overflow drops the unit,
// which is scanned again as two halves of the span, or -- one rank -- as two halves of the window.  One rank and <= R positions
// cannot overflow a bucket of R entries: the result never depends on R or on the bucket size.
#include "ivf_units.h"
#include "pq_kernels.h"

#include <algorithm>
#include <cstring>
#include <functional>

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
struct IvfpqScan {
	const unsigned char *codes; // list-sorted rows of `pitch` bytes
	const long long *lids;      // their stored ids
	const long long *list_off;  // [nlist + 1]
	const float *cent;          // [nlist][d]
	const float *cb;            // [M][256][dsub]
	const float *xq;            // the chunk's queries [nqc][d]
	const unsigned *pref;       // the chunk's ordinal bases [nqc][np + 1]
	const int2 *pairs;          // the unit's (query, rank) pairs grouped by list
	const int *poff, *goff;     // [nlist + 1]
	const unsigned *thr;        // [nqc] bounds
	unsigned long long *bucket; // [nqc][R]
	unsigned *cnt;              // [nqc]
	int *overflow;
	const long long *idmap;
	int nlist, d, M, dsub, pitch, G, np, is_l2;
	long long p0, p1; // the unit's position window
	SelectorDev sel;
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
			const float *cbj = a.cb + ((size_t)m * PQ_KSUB + j) * dsub;
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
	for (int gq = 0; gq < a.G; ++gq) {
		const int sg0 = gq * W;
		if (sg0 >= npg)
			break;
		unsigned th[W], ob[W];
		int qq[W];
		float b0[W];
#pragma unroll
		for (int w = 0; w < W; ++w) {
			const bool valid = sg0 + w < npg;
			qq[w] = valid ? s_q[sg0 + w] : 0;
			th[w] = valid ? a.thr[qq[w]] : 0u; // (0: no key is below it -- a slot without a pair admits nothing)
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
				const unsigned key = pq_key(acc[w], descending);
				if (key < th[w]) {
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

// ---------------------------------------------------------------------------------------------- emit
__global__ __launch_bounds__(256) void ivfpq_emit_kernel(const unsigned long long *__restrict__ list, const int *__restrict__ len, int k, long long nqc,
                                                         int descending, const long long *__restrict__ cI, int np, const unsigned *__restrict__ pref,
                                                         const long long *__restrict__ list_off, const long long *__restrict__ lids,
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
		const long long id = lids[list_off[cI[q * np + lo]] + (ord - pq[lo])];
		D[i] = pq_unkey((unsigned)(e >> 32), descending);
		I[i] = idmap ? idmap[id] : id;
	} else {
		D[i] = descending ? -FLT_MAX : FLT_MAX;
		I[i] = -1;
	}
}

// ---------------------------------------------------------------------------------------------- index
class IVFPQIndex : public IndexBase {
public:
	FlatIndex *quantizer; // owned; nlist centroids
	const int64_t nlist;
	const int M, dsub, pitch; // pitch: code bytes per row in the stores, M rounded up to 16
	int64_t nprobe = 1;
	bool have_cb = false;
	float *d_cb = nullptr;            // [M][256][dsub]
	unsigned char *d_codes = nullptr; // [cap][pitch] arrival order
	int64_t cap = 0;
	std::vector<int32_t> assign_h;
	std::vector<int64_t> ids_h;
	// the list-sorted view, rebuilt lazily
	bool dirty = true, cent_dirty = true;
	std::vector<int64_t> list_off, sid_h, top_rows; // top_rows[i]: rows of the i largest lists together
	int64_t nsorted = 0, max_list = 0;
	DevBuf lcodes, lids, list_off_dev, cent_dev;
	DevBuf ws_add, ws_res, ws_lab, ws_cD, ws_cI, ws_pref, ws_pairs, ws_grp, ws_bucket, ws_list, ws_ctl;
	int *h_flag = nullptr; // pinned
	SelectorHolder selector;
	int64_t last_launches = 0, last_rescans = 0;

	IVFPQIndex(int d_, int64_t nlist_, int M_, int metric_)
	    : IndexBase(MVS_KIND_IVFPQ, d_, metric_), nlist(nlist_), M(M_), dsub(d_ / M_), pitch((M_ + 15) / 16 * 16) {
		if (metric != METRIC_L2 && metric != METRIC_IP)
			throw_faiss("mvs::IVFPQIndex", __FILE__, "metric type %d is not implemented on the MI355X path", metric);
		quantizer = new FlatIndex(d, metric);
		is_trained = false;
	}
	~IVFPQIndex() override {
		(void)hipSetDevice(device);
		if (stream)
			(void)hipStreamSynchronize(stream);
		free_device();
		delete quantizer;
	}
	void free_device() {
		if (d_cb)
			(void)hipFree(d_cb);
		if (d_codes)
			(void)hipFree(d_codes);
		if (h_flag)
			(void)hipHostFree(h_flag);
		d_cb = nullptr, d_codes = nullptr, h_flag = nullptr, cap = 0;
		for (DevBuf *b : {&lcodes, &lids, &list_off_dev, &cent_dev, &ws_add, &ws_res, &ws_lab, &ws_cD, &ws_cI, &ws_pref, &ws_pairs, &ws_grp, &ws_bucket,
		                  &ws_list, &ws_ctl})
			b->release();
		selector.buf.release();
		dirty = cent_dirty = true;
	}
	size_t cb_floats() const {
		return (size_t)M * PQ_KSUB * dsub;
	}
	void adopt_tuning(const Tuning &t) override {
		tune_ = t;
		quantizer->adopt_tuning(t);
	}

	// ------------------------------------------------------------------------------------------ train
	void check_empty_for_training() const {
		if (ntotal > 0)
			throw_faiss("mvs::IVFPQIndex::train", __FILE__, "the index already holds %lld rows encoded with its centroids and codebooks: "
			            "training again is only possible while it is empty", (long long)ntotal);
	}
	void update_trained() {
		is_trained = have_cb && quantizer->ntotal == nlist;
	}
	void set_coarse(const float *c) {
		use_device();
		check_empty_for_training();
		quantizer->reset();
		quantizer->add(nlist, c);
		cent_dirty = true;
		update_trained();
	}
	void set_codebooks(const float *c) {
		use_device();
		check_empty_for_training();
		if (!d_cb)
			MVS_HIP(hipMalloc((void **)&d_cb, cb_floats() * sizeof(float)));
		MVS_HIP(hipMemcpyAsync(d_cb, c, cb_floats() * sizeof(float), hipMemcpyHostToDevice, stream));
		MVS_HIP(hipStreamSynchronize(stream));
		have_cb = true;
		update_trained();
	}
	void get_coarse(float *out) {
		use_device();
		HostIndex h;
		quantizer->to_host(h);
		memcpy(out, h.rows.data(), h.rows.size() * sizeof(float));
	}
	void get_codebooks(float *out) {
		use_device();
		if (!d_cb)
			throw_faiss("mvs::IVFPQIndex::get_centroids", __FILE__, "the index has no codebooks yet");
		MVS_HIP(hipStreamSynchronize(stream));
		MVS_HIP(hipMemcpy(out, d_cb, cb_floats() * sizeof(float), hipMemcpyDeviceToHost));
	}
	const float *centroids_dev() { // [nlist][d] row-major copy of the quantiser's rows (on `stream`)
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
		{ // 1. the coarse centroids: IVF<n>,Flat of the same metric (spherical under inner product, as there)
			std::unique_ptr<IndexBase> iv(make_ivf_index(d, "IVF" + std::to_string(nlist) + ",Flat", metric));
			iv->adopt_tuning(tune_);
			iv->train(n, x);
			std::vector<float> cent((size_t)nlist * d);
			ivf_get_centroids(iv.get(), cent.data());
			have_cb = false;
			set_coarse(cent.data());
		}
		// 2. every training row's residual against its k = 1 centroid, in input order
		std::vector<float> res((size_t)n * d);
		const int64_t bs = 65536;
		ws_add.reserve((size_t)std::min(bs, n) * d * sizeof(float));
		ws_res.reserve((size_t)std::min(bs, n) * d * sizeof(float));
		ws_lab.reserve((size_t)std::min(bs, n) * (sizeof(float) + sizeof(int64_t)));
		for (int64_t i0 = 0; i0 < n; i0 += bs) {
			const int64_t nb = std::min(bs, n - i0);
			MVS_HIP(hipMemcpyAsync(ws_add.p, x + i0 * d, (size_t)nb * d * sizeof(float), hipMemcpyHostToDevice, stream));
			int64_t *d_lab = (int64_t *)ws_lab.p;
			assign_device(nb, (const float *)ws_add.p, (float *)(d_lab + nb), d_lab);
			residuals_device(nb, (const float *)ws_add.p, d_lab, (float *)ws_res.p);
			MVS_HIP(hipMemcpyAsync(&res[(size_t)i0 * d], ws_res.p, (size_t)nb * d * sizeof(float), hipMemcpyDeviceToHost, stream));
			MVS_HIP(hipStreamSynchronize(stream));
		}
		// 3. codebook m: IVF256,Flat (L2) on the residuals' columns [m dsub, (m+1) dsub) -- also under inner product
		std::vector<float> cent(cb_floats()), cols((size_t)n * dsub);
		for (int m = 0; m < M; ++m) {
			for (int64_t i = 0; i < n; ++i)
				memcpy(&cols[(size_t)i * dsub], &res[(size_t)i * d + (size_t)m * dsub], (size_t)dsub * sizeof(float));
			std::unique_ptr<IndexBase> iv(make_ivf_index(dsub, "IVF256,Flat", METRIC_L2));
			iv->adopt_tuning(tune_);
			iv->train(n, cols.data());
			ivf_get_centroids(iv.get(), &cent[(size_t)m * PQ_KSUB * dsub]);
		}
		set_codebooks(cent.data());
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
		if (ntotal > 0 && off != label_offset)
			throw_faiss("mvs::IVFPQIndex::set_label_offset", __FILE__, "the label offset of an IVF index must be set before rows are added");
		label_offset = off;
	}
	// d_x: [n][d] rows on the device, in `stream` order; ids (host) may be null
	void add_core_device(int64_t n, const float *d_x, const int64_t *ids_host) {
		if (!is_trained)
			throw_faiss("virtual void faiss::IndexIVFPQ::add_core(...)", "faiss/IndexIVFPQ.cpp", "Error: 'is_trained' failed");
		if (ntotal + n > (int64_t)0x7fffffff - 1024)
			throw_faiss("mvs::IVFPQIndex::add", __FILE__, "a single-device index holds at most 2^31 rows");
		grow(ntotal + n);
		const int64_t bs = 65536; // IndexIVF::add_with_ids block size
		ws_res.reserve((size_t)std::min(bs, n) * d * sizeof(float));
		ws_lab.reserve((size_t)std::min(bs, n) * (sizeof(float) + sizeof(int64_t)));
		std::vector<int64_t> lab((size_t)std::min(bs, n));
		assign_h.reserve((size_t)(ntotal + n));
		ids_h.reserve((size_t)(ntotal + n));
		const bool in_lds = dsub <= PQ_ENCODE_LDS_DSUB;
		const size_t lds = in_lds ? (size_t)2 * PQ_KSUB * dsub * sizeof(float) : 0;
		if (lds > (48u << 10))
			ensure_dynamic_lds((const void *)pq_encode_kernel, lds);
		for (int64_t i0 = 0; i0 < n; i0 += bs) {
			const int64_t nb = std::min(bs, n - i0);
			int64_t *d_lab = (int64_t *)ws_lab.p;
			assign_device(nb, d_x + i0 * d, (float *)(d_lab + nb), d_lab);
			MVS_HIP(hipMemcpyAsync(lab.data(), d_lab, (size_t)nb * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
			residuals_device(nb, d_x + i0 * d, d_lab, (float *)ws_res.p);
			hipLaunchKernelGGL(pq_encode_kernel, dim3((unsigned)((nb + 255) / 256), (unsigned)M), dim3(256), lds, stream, (const float *)ws_res.p,
			                   (long long)nb, d, dsub, (const float *)d_cb, d_codes, pitch, (long long)(ntotal + i0), in_lds ? 1 : 0);
			MVS_HIP(hipGetLastError());
			MVS_HIP(hipStreamSynchronize(stream));
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
		if (!is_trained) // (before the rows travel)
			throw_faiss("virtual void faiss::IndexIVFPQ::add_core(...)", "faiss/IndexIVFPQ.cpp", "Error: 'is_trained' failed");
		ws_add.reserve((size_t)n * d * sizeof(float));
		MVS_HIP(hipMemcpyAsync(ws_add.p, x, (size_t)n * d * sizeof(float), hipMemcpyHostToDevice, stream));
		add_core_device(n, (const float *)ws_add.p, ids);
	}
	void add(int64_t n, const float *x) override {
		add_host(n, x, nullptr);
	}
	void add_with_ids(int64_t n, const float *x, const int64_t *ids) override {
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
		use_device();
		if (n <= 0)
			return;
		stream_wait(stream, st);
		std::vector<int64_t> ids((size_t)n);
		MVS_HIP(hipMemcpy(ids.data(), d_ids, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
		add_core_device(n, d_x, ids.data());
	}

	// ------------------------------------------------------------------------------------------ list view
	// rows grouped by list, arrival order inside a list (ArrayInvertedLists semantics): codes gathered on the device
	void build_lists() {
		if (!dirty)
			return;
		list_off.assign((size_t)nlist + 1, 0);
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
		list_off_dev.reserve(list_off.size() * sizeof(int64_t));
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
		MVS_HIP(hipMemcpyAsync(list_off_dev.p, list_off.data(), list_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
		MVS_HIP(hipStreamSynchronize(stream));
		dirty = false;
	}
	int64_t list_size(int64_t l) {
		use_device();
		if (l < 0 || l >= nlist)
			throw_faiss("mvs::IVFPQIndex::list_size", __FILE__, "list %lld is outside [0, %lld)", (long long)l, (long long)nlist);
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
			MVS_HIP(hipMemcpy2D(codes, (size_t)M, (const unsigned char *)lcodes.p + (size_t)b * pitch, (size_t)pitch, (size_t)M, (size_t)n, hipMemcpyDeviceToHost));
	}

	// ------------------------------------------------------------------------------------------ search
	struct Chunk { // one chunk of queries: device state of its selection, the scan's fixed arguments
		int64_t nqc;
		int k, W, G, np;
		const int64_t *cI;
		unsigned long long *list;
		int *len, *gcnt, *gcur, *poff, *goff;
		IvfpqScan a;
	};
	// the rows one query can send to its bucket from a unit, at most
	int64_t unit_rows(int ra, int rb, int64_t p0, int64_t p1) const {
		if (rb - ra == 1)
			return std::min(max_list, p1) - p0;
		return top_rows[(size_t)std::min<int64_t>(rb - ra, nlist) - 1];
	}
	void launch_scan(Chunk &c, int ra, int rb, int64_t p0, int64_t p1) {
		const int Q = c.W * c.G, span = rb - ra;
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
		const int64_t gy = (std::min(max_list, p1) - p0 + IVFPQ_ROWS_PER_WG - 1) / IVFPQ_ROWS_PER_WG;
		const dim3 grid((unsigned)gx, (unsigned)gy);
		const size_t lds = (size_t)Q * M * PQ_KSUB * sizeof(float) + (size_t)IVFPQ_VSTAGE_FLOATS * sizeof(float) + (size_t)3 * IVFPQ_MAX_Q * sizeof(float);
		c.a.p0 = p0, c.a.p1 = p1;
		begin_kernel_timing(stream);
#define IVFPQ_LAUNCH_SCAN(WW)                                                                                                                       \
	do {                                                                                                                                            \
		ensure_dynamic_lds((const void *)ivfpq_scan_kernel<WW>, lds);                                                                               \
		hipLaunchKernelGGL(ivfpq_scan_kernel<WW>, grid, dim3(PQ_SCAN_THREADS), lds, stream, c.a);                                                   \
	} while (0)
		if (c.W == 4)
			IVFPQ_LAUNCH_SCAN(4);
		else if (c.W == 2)
			IVFPQ_LAUNCH_SCAN(2);
		else
			IVFPQ_LAUNCH_SCAN(1);
#undef IVFPQ_LAUNCH_SCAN
		MVS_HIP(hipGetLastError());
		end_kernel_timing(stream);
		const double rows = (double)unit_rows(ra, rb, p0, p1);
		set_kinfo("ivfpq_scan_kernel", (double)c.nqc * rows * M, (double)c.nqc * rows * M / Q, (int)(gx * gy), PQ_SCAN_THREADS, (int)lds, (int)gy);
		++last_launches;
	}
	// ranks [ra, rb), positions [p0, p1) of their lists, into every list of the chunk
	void scan_unit(Chunk &c, int ra, int rb, int64_t p0, int64_t p1) {
		launch_scan(c, ra, rb, p0, p1);
		if (unit_rows(ra, rb, p0, p1) > IVFPQ_ROWS_PER_WG) { // (a unit of at most R rows per query cannot overflow a bucket of R entries)
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
					const int64_t mid = p0 + ((w1 - p0) / 2 + IVFPQ_ROWS_PER_WG - 1) / IVFPQ_ROWS_PER_WG * IVFPQ_ROWS_PER_WG;
					scan_unit(c, ra, rb, p0, mid);
					scan_unit(c, ra, rb, mid, w1);
				}
				return;
			}
		}
		int P = 1;
		while (P < c.k + IVFPQ_ROWS_PER_WG)
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
		if (k <= 0)
			throw_faiss("virtual void faiss::IndexIVF::search(...) const", "faiss/IndexIVF.cpp", "Error: 'k > 0' failed");
		if (k > PQ_MAX_K)
			throw_faiss("mvs::IVFPQIndex::search", __FILE__, "k = %lld is beyond the largest k the IVFPQ index serves on the MI355X path (%d)",
			            (long long)k, PQ_MAX_K);
		if (!is_trained)
			throw_faiss("virtual void faiss::IndexIVF::search(...) const", "faiss/IndexIVF.cpp", "Error: 'is_trained' failed");
		if (nq <= 0)
			return;
		int64_t np = params && params->nprobe > 0 ? params->nprobe : nprobe;
		np = std::min(np, nlist); // IndexIVF::search: nprobe = min(nlist, params->nprobe)
		if (np <= 0)
			throw_faiss("virtual void faiss::IndexIVF::search(...) const", "faiss/IndexIVF.cpp", "Error: 'nprobe > 0' failed");
		stream_wait(stream, st); // our stream carries the adds and the list view; the caller's the queries
		build_lists();
		const float *d_cent = centroids_dev();
		const int W = pq_width(M), G = pq_groups(M);
		// 1. the probed lists of the whole batch, the ordinal bases
		ws_cD.reserve((size_t)nq * np * sizeof(float));
		ws_cI.reserve((size_t)nq * np * sizeof(int64_t));
		ws_pref.reserve((size_t)nq * (np + 1) * sizeof(unsigned));
		if (nsorted > 0) {
			if (!quantizer->coarse_topk(nq, d_x, np, (float *)ws_cD.p, (int64_t *)ws_cI.p, stream, false))
				quantizer->search_device(nq, d_x, np, (float *)ws_cD.p, (int64_t *)ws_cI.p, nullptr, stream);
			use_device();
			hipLaunchKernelGGL(ivfpq_prefix_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, (const long long *)ws_cI.p, (long long)nq,
			                   (int)np, (const long long *)list_off_dev.p, (long long)nlist, (unsigned *)ws_pref.p);
			MVS_HIP(hipGetLastError());
		}
		// 2. queries per chunk: buckets <= 256 MB
		const int64_t nqc_max = std::min<int64_t>(nq, (int64_t)(PQ_BUCKET_SCRATCH / ((size_t)IVFPQ_ROWS_PER_WG * sizeof(unsigned long long))));
		int np_span = 1; // the widest rank span a unit can have
		for (int ra = 0, rb = 1; ra < np; ra = rb, rb = (int)std::min<int64_t>(np, 3 * (int64_t)rb))
			np_span = std::max(np_span, rb - ra);
		ws_bucket.reserve((size_t)nqc_max * IVFPQ_ROWS_PER_WG * sizeof(unsigned long long));
		ws_list.reserve((size_t)nqc_max * k * sizeof(unsigned long long));
		ws_pairs.reserve((size_t)nqc_max * np_span * sizeof(int2));
		ws_grp.reserve((size_t)(4 * nlist + 2) * sizeof(int)); // cnt [nlist] | cur [nlist] | poff [nlist + 1] | goff [nlist + 1]
		// control block: len [nqc] | cnt [nqc] | overflow (+ pad) | thr [nqc]
		const size_t ctl_zero = (size_t)(2 * nqc_max + 4) * sizeof(int);
		ws_ctl.reserve(ctl_zero + (size_t)nqc_max * sizeof(unsigned));
		if (!h_flag)
			MVS_HIP(hipHostMalloc((void **)&h_flag, sizeof(int), hipHostMallocDefault));
		Chunk c;
		c.k = (int)k, c.W = W, c.G = G, c.np = (int)np;
		c.list = (unsigned long long *)ws_list.p;
		c.len = (int *)ws_ctl.p;
		c.gcnt = (int *)ws_grp.p;
		c.gcur = c.gcnt + nlist;
		c.poff = c.gcur + nlist;
		c.goff = c.poff + nlist + 1;
		IvfpqScan &a = c.a;
		a.codes = (const unsigned char *)lcodes.p;
		a.lids = (const long long *)lids.p;
		a.list_off = (const long long *)list_off_dev.p;
		a.cent = d_cent;
		a.cb = d_cb;
		a.pairs = (const int2 *)ws_pairs.p;
		a.poff = c.poff, a.goff = c.goff;
		a.bucket = (unsigned long long *)ws_bucket.p;
		a.cnt = (unsigned *)ws_ctl.p + nqc_max;
		a.overflow = (int *)ws_ctl.p + 2 * nqc_max;
		a.thr = (unsigned *)((char *)ws_ctl.p + ctl_zero);
		a.idmap = (const long long *)d_idmap;
		a.nlist = (int)nlist, a.d = d, a.M = M, a.dsub = dsub, a.pitch = pitch, a.G = G, a.np = (int)np, a.is_l2 = metric == METRIC_L2 ? 1 : 0;
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
				for (int ra = 0, rb = 1; ra < np; ra = rb, rb = (int)std::min<int64_t>(np, 3 * (int64_t)rb))
					scan_unit(c, ra, rb, 0, max_list);
			const int64_t tot = c.nqc * k;
			hipLaunchKernelGGL(ivfpq_emit_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, (const unsigned long long *)c.list,
			                   (const int *)c.len, c.k, (long long)c.nqc, metric == METRIC_IP ? 1 : 0, (const long long *)c.cI, (int)np, a.pref,
			                   (const long long *)list_off_dev.p, (const long long *)lids.p, raw_labels ? nullptr : (const long long *)d_idmap, d_D + q0 * k, // (raw_labels: csrc/index.h)
			                   (long long *)(d_I + q0 * k));
			MVS_HIP(hipGetLastError());
		}
		stream_wait(st, stream);
	}
	void search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, hipStream_t st) override {
		search_mapped(nq, d_x, k, d_D, d_I, params, nullptr, st);
	}
	bool named_stat(const char *name, int64_t *value) override {
		if (!strcmp(name, "ivfpq_pair_block"))
			*value = pq_width(M) * pq_groups(M);
		else if (!strcmp(name, "ivfpq_rows_per_workgroup"))
			*value = IVFPQ_ROWS_PER_WG;
		else if (!strcmp(name, "ivfpq_scan_launches"))
			*value = last_launches;
		else if (!strcmp(name, "ivfpq_scan_rescans"))
			*value = last_rescans;
		else
			return false;
		return true;
	}
	size_t device_bytes() const override {
		return (size_t)cap * pitch + lcodes.cap + lids.cap + (d_cb ? cb_floats() * sizeof(float) : 0);
	}

	// ------------------------------------------------------------------------------------------ images, placement
	// ArrayInvertedLists image: per list, M-byte codes and ids in arrival order
	void to_host(HostIndex &out) override {
		use_device();
		MVS_HIP(hipStreamSynchronize(stream));
		build_lists();
		out.kind = MVS_KIND_IVFPQ;
		out.d = d;
		out.metric = metric;
		out.metric_arg = metric_arg;
		out.ntotal = ntotal;
		out.is_trained = is_trained;
		out.nlist = nlist;
		out.nprobe = nprobe;
		out.sub.reset(new HostIndex);
		quantizer->to_host(*out.sub);
		out.pq_M = M;
		out.pq_centroids.assign(cb_floats(), 0.f); // (FAISS allocates the codebooks with the ProductQuantizer: an image without them holds zeros)
		if (have_cb)
			get_codebooks(out.pq_centroids.data());
		std::vector<uint8_t> all((size_t)nsorted * M);
		if (nsorted > 0)
			MVS_HIP(hipMemcpy2D(all.data(), (size_t)M, lcodes.p, (size_t)pitch, (size_t)M, (size_t)nsorted, hipMemcpyDeviceToHost));
		out.list_ids.assign((size_t)nlist, {});
		out.list_bytes.assign((size_t)nlist, {});
		for (int64_t l = 0; l < nlist; l++) {
			const int64_t b = list_off[(size_t)l], e = list_off[(size_t)l + 1];
			out.list_ids[(size_t)l].assign(sid_h.begin() + b, sid_h.begin() + e);
			out.list_bytes[(size_t)l].assign(all.begin() + b * M, all.begin() + e * M);
		}
	}
	// an empty index on its device <- codebooks and lists of the image (the quantiser is loaded by the caller); rows enter in list
	// order, which keeps the arrival order inside every list
	void load_image(const HostIndex &h) {
		if ((int64_t)h.list_ids.size() != nlist || (int64_t)h.list_bytes.size() != nlist || h.pq_centroids.size() != cb_floats())
			throw_faiss("faiss::Index* faiss::read_index(...)", "faiss/impl/index_read.cpp", "IVFPQ image: inverted lists or codebooks do not match "
			            "nlist = %lld, d = %d, M = %d", (long long)nlist, d, M);
		int64_t n = 0;
		for (int64_t l = 0; l < nlist; l++) {
			if (h.list_bytes[(size_t)l].size() != h.list_ids[(size_t)l].size() * (size_t)M)
				throw_faiss("faiss::Index* faiss::read_index(...)", "faiss/impl/index_read.cpp", "IVFPQ image: list %lld holds %zu code bytes for %zu ids",
				            (long long)l, h.list_bytes[(size_t)l].size(), h.list_ids[(size_t)l].size());
			n += (int64_t)h.list_ids[(size_t)l].size();
		}
		if (n > (int64_t)0x7fffffff - 1024)
			throw_faiss("mvs::IVFPQIndex::add", __FILE__, "a single-device index holds at most 2^31 rows");
		use_device();
		metric_arg = h.metric_arg;
		nprobe = h.nprobe;
		bool any = false;
		for (float v : h.pq_centroids)
			any = any || v != 0.f;
		if (h.is_trained || any)
			set_codebooks(h.pq_centroids.data());
		cent_dirty = true;
		update_trained();
		grow(n);
		std::vector<uint8_t> all((size_t)n * M);
		assign_h.clear();
		ids_h.clear();
		int64_t r = 0;
		for (int64_t l = 0; l < nlist; l++) {
			const auto &li = h.list_ids[(size_t)l];
			if (!li.empty())
				memcpy(&all[(size_t)r * M], h.list_bytes[(size_t)l].data(), li.size() * (size_t)M);
			for (size_t j = 0; j < li.size(); j++, r++) {
				assign_h.push_back((int32_t)l);
				ids_h.push_back(li[j]);
			}
		}
		if (n > 0)
			MVS_HIP(hipMemcpy2D(d_codes, (size_t)pitch, all.data(), (size_t)M, (size_t)M, (size_t)n, hipMemcpyHostToDevice));
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
		have_cb = false;
		ws_hx.release();
		ws_hD.release();
		ws_hI.release();
		MVS_HIP(hipStreamDestroy(stream));
		stream = nullptr;
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
		IndexBase *c = ivfpq_from_host(img, on_device);
		c->label_offset = label_offset;
		return c;
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
			p->quantizer->add(h.sub->ntotal, h.sub->rows.data());
		p->load_image(h);
	} catch (...) {
		delete p;
		throw;
	}
	return p;
}
IndexBase *ivfpq_quantizer_of(IndexBase *ix) {
	IVFPQIndex *p = as_ivfpq(ix);
	return p ? p->quantizer : nullptr;
}
int64_t ivfpq_nlist_of(IndexBase *ix) {
	IVFPQIndex *p = as_ivfpq(ix);
	return p ? p->nlist : 0;
}
bool ivfpq_get_coarse(IndexBase *ix, float *out) {
	IVFPQIndex *p = as_ivfpq(ix);
	if (p)
		p->get_coarse(out);
	return p != nullptr;
}
bool ivfpq_set_coarse(IndexBase *ix, const float *c) {
	IVFPQIndex *p = as_ivfpq(ix);
	if (p)
		p->set_coarse(c);
	return p != nullptr;
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
int64_t ivfpq_list_size(IndexBase *ix, int64_t list_no) {
	IVFPQIndex *p = as_ivfpq(ix);
	if (!p)
		throw_faiss("mvs_index_ivfpq_list_size", __FILE__, "not an IVFPQ index");
	return p->list_size(list_no);
}
void ivfpq_get_list(IndexBase *ix, int64_t list_no, int64_t *ids, uint8_t *codes) {
	IVFPQIndex *p = as_ivfpq(ix);
	if (!p)
		throw_faiss("mvs_index_ivfpq_get_list", __FILE__, "not an IVFPQ index");
	p->get_list(list_no, ids, codes);
}

} // namespace mvs
