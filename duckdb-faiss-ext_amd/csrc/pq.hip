// csrc/pq.hip -- product-quantised index "PQ<M>" (faiss::IndexPQ, the dynamic_cast target of src/faiss_extension.cpp:704), 8 bits per code.
//
// Contract (include/mi355_faiss.h "product-quantised indexes", DESIGN.md "PQ"):
//   train   codebook m = the centroids IVF256,Flat (L2) learns from columns [m dsub, (m+1) dsub) -- the index's own device k-means
//   encode  code[i][m] = argmin_j of the pair-path L2 chain acc = fmaf(t, t, acc), t = x[k] - c[k], k ascending; smallest j on a tie
//   search  T[q][m][j] = that chain (L2) or the ip chain fmaf(x[k], c[k], acc) (inner product); dis(q, i) = sum over m ascending of
//           T[q][m][code[i][m]] in f32; the k best in the PURE order: distance (L2 ascending, inner product descending), then row number
//   admission  ... among the values FAISS's heap can hold (csrc/pq_kernels.h "ADMISSION RULE"): a NaN sum, and a sum not strictly better
//           than FLT_MAX (L2: +inf, an overflowed sum) / -FLT_MAX (inner product: -inf), is never a result; its slot is (-1, +-FLT_MAX)
//
// Kernels
//   (pq_encode_kernel and pq_select_kernel live in csrc/pq_kernels.h: csrc/ivfpq.hip runs them too)
//   pq_encode_kernel   one workgroup = 256 rows x one sub-space, the sub-space's codebook in LDS (dsub <= 64; beyond that it is read
//                      through the caches), one lane per (row, m), one byte out
//   pq_tables_kernel   the tables of one CHUNK of queries (<= 64 MB), written in the layout the scan's LDS image has
//   pq_scan_kernel<W>  the hot path: a workgroup holds the tables of Q = W G queries in LDS, W of them interleaved per (m, j) entry --
//                      float4 for M <= 32, float2 for M <= 64, scalar up to M = 128 -- so that one ds_read_b128 / b64 gather serves W
//                      (query, row) pairs; a lane walks its rows' code bytes and adds the entries up, m ascending.  No k-lists: a sum that
//                      beats its query's bound goes to the query's bucket in a candidate stream
//   pq_select_kernel   one workgroup per query: its list so far + its bucket, sorted as (order key, row) 64-bit keys in LDS; the first k
//                      stay, the k-th key becomes the bound
//   pq_emit_kernel     keys -> distances and labels (IDMap: id_map[row]), -1 / FLT_MAX padded
//
// Selection.  Rows are scanned in RANGES of ascending row numbers: [0, R), [R, 3R), [3R, 9R), ...  (R = rows per workgroup = bucket
// size).  After a range every query's list holds the k best rows seen so far in the pure order, so a later row -- whose number exceeds
// all of them -- can only enter with a key STRICTLY below the k-th: rows tied at the bound never reach the stream, and among ties the
// lowest rows survive by construction.  Rows in random order send about 2k candidates per query and range.  A bucket that overflows
// (rows arriving best-last) raises a flag; the range is then scanned again in two halves, down to ranges of R rows, which cannot
// overflow -- the result never depends on the bucket size.
// Before its first range a query's bound is PQ_OPEN_BOUND, the key of the heap's neutral element: what is not strictly better never enters.
#include "coded_lists.h"
#include "pq_kernels.h"

#include <cfloat>
#include <cstring>

namespace mvs {

namespace {

// ---------------------------------------------------------------------------------------------- tables
// T [query block][group][m][j][w]: query q of the chunk is block q / (W G), group (q % (W G)) / W, lane w = q % W
__global__ __launch_bounds__(256) void pq_tables_kernel(const float *__restrict__ xq, int d, int M, int dsub, const float *__restrict__ cb, int is_l2,
                                                        int W, int G, float *__restrict__ T) {
	const long long q = blockIdx.x;
	const int m = blockIdx.y, j = threadIdx.x;
	const float *xv = xq + q * d + (long long)m * dsub;
	const float *c = cb + ((size_t)m * PQ_KSUB + j) * dsub;
	float acc = 0.f;
	if (is_l2) {
		for (int k = 0; k < dsub; ++k) {
			const float t = xv[k] - c[k];
			acc = fmaf(t, t, acc);
		}
	} else {
		for (int k = 0; k < dsub; ++k)
			acc = fmaf(xv[k], c[k], acc);
	}
	const int Q = W * G;
	const long long b = q / Q;
	const int r = (int)(q - b * Q), g = r / W, w = r - g * W;
	T[((((size_t)b * G + g) * M + m) * PQ_KSUB + j) * W + w] = acc;
}

// ---------------------------------------------------------------------------------------------- scan
// rows [r0, r1) against the queries of block blockIdx.y; workgroup blockIdx.x walks rows r0 + blockIdx.x R ... (+ R)
template <int W>
__global__ __launch_bounds__(PQ_SCAN_THREADS) void pq_scan_kernel(const unsigned char *__restrict__ codes, int pitch, int M, long long r0, long long r1,
                                                                  const float *__restrict__ T, int G, long long nqc, const unsigned *__restrict__ thr,
                                                                  unsigned long long *__restrict__ bucket, unsigned *__restrict__ cnt, int *__restrict__ overflow,
                                                                  int descending, SelectorDev sel, const long long *__restrict__ idmap) {
	extern __shared__ float4 pq_scan_lds[];
	typedef typename PqEntry<W>::type entry_t;
	const int tid = threadIdx.x, Q = W * G;
	const unsigned smask = pq_sign_mask(descending);
	const long long qb = blockIdx.y;
	const size_t tvec = (size_t)Q * M * PQ_KSUB / 4; // float4s of the block's tables (Q M 256 floats, a multiple of 4)
	const float4 *src = reinterpret_cast<const float4 *>(T) + (size_t)qb * tvec;
	for (size_t i = tid; i < tvec; i += PQ_SCAN_THREADS)
		pq_scan_lds[i] = src[i];
	__syncthreads();
	const long long wg0 = r0 + (long long)blockIdx.x * PQ_ROWS_PER_WG;
	const long long wg1 = wg0 + PQ_ROWS_PER_WG < r1 ? wg0 + PQ_ROWS_PER_WG : r1;
	for (int g = 0; g < G; ++g) {
		const long long q0 = qb * Q + (long long)g * W;
		if (q0 >= nqc)
			break;
		float th[W]; // the bounds as values (pq_bound_value)
#pragma unroll
		for (int w = 0; w < W; ++w)
			th[w] = pq_bound_value(q0 + w < nqc ? thr[q0 + w] : 0u, descending); // (0: no key is below it -- a query past the chunk's end admits nothing)
		const entry_t *Tg = reinterpret_cast<const entry_t *>(pq_scan_lds) + (size_t)g * M * PQ_KSUB;
		for (long long row = wg0 + tid; row < wg1; row += PQ_SCAN_THREADS) {
			if (sel.kind != MVS_SEL_NONE && !pq_sel_member(sel, idmap ? idmap[row] : row))
				continue;
			const uint4 *cr = reinterpret_cast<const uint4 *>(codes + row * pitch);
			float acc[W];
#pragma unroll
			for (int w = 0; w < W; ++w)
				acc[w] = 0.f; // (0 + T is T bit for bit: no entry is -0, both chains start from +0)
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
					const unsigned pos = atomicAdd(&cnt[q0 + w], 1u);
					if (pos < (unsigned)PQ_ROWS_PER_WG)
						bucket[(size_t)(q0 + w) * PQ_ROWS_PER_WG + pos] = ((unsigned long long)key << 32) | (unsigned long long)(unsigned)row;
					else
						*overflow = 1;
				}
			}
		}
	}
}

// ---------------------------------------------------------------------------------------------- emit
__global__ __launch_bounds__(256) void pq_emit_kernel(const unsigned long long *__restrict__ list, const int *__restrict__ len, int k, long long nqc,
                                                      int descending, const long long *__restrict__ idmap, long long label_offset,
                                                      float *__restrict__ D, long long *__restrict__ I) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nqc * k)
		return;
	const long long q = i / k;
	const int s = (int)(i - q * k);
	if (s < len[q]) {
		const unsigned long long e = list[i];
		const long long row = (long long)(e & 0xFFFFFFFFull);
		D[i] = pq_unkey((unsigned)(e >> 32), descending);
		I[i] = idmap ? idmap[row] : row + label_offset;
	} else {
		D[i] = descending ? -FLT_MAX : FLT_MAX;
		I[i] = -1;
	}
}

// ---------------------------------------------------------------------------------------------- index
// Every device workspace a PQIndex keeps between calls, and nothing else (as FlatWork, csrc/index.h: a DevBuf added here and left out
// of release_all() does not compile)
struct PQWork {
	DevBuf ws_add, ws_T, ws_bucket, ws_list, ws_ctl;
	void release_all() { // the index leaves its device (PQIndex::to_device)
		DevBuf *const all[] = {&ws_add, &ws_T, &ws_bucket, &ws_list, &ws_ctl};
		static_assert(sizeof all / sizeof *all * sizeof(DevBuf) == sizeof(PQWork), "a workspace of PQWork is missing from release_all()");
		for (DevBuf *b : all)
			b->release();
	}
};

class PQIndex : public IndexBase, public PQWork {
public:
	const int M, dsub;
	DevBlock<float> cb_;
	float *d_cb() const { // [M][256][dsub]; null until set_centroids
		return cb_.get();
	}
	CodeStore store;  // [cap][pitch], pitch: M rounded up to 16 (one uint4 per 16 sub-quantisers)
	PinnedMem h_flag; // one int: a scan's overflow flag
	SelectorHolder selector;
	int64_t last_ranges = 0, last_rescans = 0; // diagnostics of the last search: scan launches, of those repeated after an overflow

	PQIndex(int d_, int M_, int metric_)
	    : IndexBase(MVS_KIND_PQ, d_, metric_), M(M_), dsub(d_ / M_), store(M_) {
		if (metric != METRIC_L2 && metric != METRIC_IP)
			throw_faiss("mvs::PQIndex", __FILE__, "metric type %d is not implemented on the MI355X path", metric);
		is_trained = false;
	}
	~PQIndex() override {
		(void)hipSetDevice(device);
		if (stream)
			(void)hipStreamSynchronize(stream);
	}
	void free_device() { // the index leaves its device (to_device): load_image builds all of it again
		cb_.release();
		h_flag.release();
		store.release();
		release_all();
		selector.release();
	}
	size_t cb_floats() const {
		return (size_t)M * PQ_KSUB * dsub;
	}

	// ------------------------------------------------------------------------------------------ train
	// (FAISS retrains a populated IndexPQ and leaves its codes stale; here the codebooks are fixed once rows are encoded with them)
	void check_empty_for_training() const {
		if (ntotal > 0)
			throw_faiss("mvs::PQIndex::train", __FILE__, "the index already holds %lld rows encoded with its codebooks: training again is "
			            "only possible while it is empty", (long long)ntotal);
	}
	void set_centroids(const float *c) {
		use_device();
		check_empty_for_training();
		if (!cb_)
			cb_ = DevBlock<float>(cb_floats());
		MVS_HIP(hipMemcpyAsync(d_cb(), c, cb_floats() * sizeof(float), hipMemcpyHostToDevice, stream));
		MVS_HIP(hipStreamSynchronize(stream));
		is_trained = true;
	}
	// ProductQuantizer::train: one Clustering(dsub, 256) per sub-space, L2 (csrc/clustering.hip)
	void train(int64_t n, const float *x) override {
		use_device();
		check_empty_for_training();
		std::vector<float> cent(cb_floats()), cols((size_t)std::max<int64_t>(n, 0) * dsub);
		for (int m = 0; m < M; ++m) {
			for (int64_t i = 0; i < n; ++i)
				memcpy(&cols[(size_t)i * dsub], x + i * d + (int64_t)m * dsub, (size_t)dsub * sizeof(float));
			CtorDevice scope(device);
			FlatIndex assigner(dsub, METRIC_L2);
			assigner.adopt_tuning(tune_);
			// 10 iterations are this project's contract (include/mi355_faiss.h, tests/pq_reference.py); FAISS's ProductQuantizer::train runs 25
			kmeans_train({PQ_KSUB, 10, false}, n, cols.data(), assigner);
			assigner.copy_rows_to_host(&cent[(size_t)m * PQ_KSUB * dsub]);
		}
		set_centroids(cent.data());
	}

	// ------------------------------------------------------------------------------------------ add
	void check_add(int64_t n) {
		if (!is_trained)
			throw_faiss("virtual void faiss::IndexPQ::add(...)", "faiss/IndexFlatCodes.cpp", "Error: 'is_trained' failed");
		if (ntotal + n > (int64_t)0x7fffffff - 1024)
			throw_faiss("mvs::PQIndex::add", __FILE__, "a single-device index holds at most 2^31 rows");
	}
	void encode(int64_t n, const float *d_x, hipStream_t st) { // rows -> codes [ntotal, ntotal + n)
		const bool in_lds = dsub <= PQ_ENCODE_LDS_DSUB;
		const size_t lds = in_lds ? (size_t)2 * PQ_KSUB * dsub * sizeof(float) : 0;
		if (lds > (48u << 10))
			ensure_dynamic_lds((const void *)pq_encode_kernel, lds);
		const dim3 grid((unsigned)((n + 255) / 256), (unsigned)M);
		hipLaunchKernelGGL(pq_encode_kernel, grid, dim3(256), lds, st, d_x, (long long)n, d, dsub, d_cb(), store.codes(), store.pitch, (long long)ntotal,
		                   in_lds ? 1 : 0);
		MVS_HIP(hipGetLastError());
	}
	void add(int64_t n, const float *x) override {
		use_device();
		if (n <= 0)
			return;
		check_add(n);
		store.grow(ntotal + n, ntotal, stream);
		const int64_t step = std::max<int64_t>(1, (int64_t)PinnedRing::SLOT_BYTES / ((int64_t)d * (int64_t)sizeof(float)));
		ws_add.reserve((size_t)std::min(step, n) * d * sizeof(float));
		for (int64_t i0 = 0; i0 < n; i0 += step) {
			const int64_t nb = std::min(step, n - i0);
			const size_t bytes = (size_t)nb * d * sizeof(float);
			const int slot = pinned.acquire(bytes);
			memcpy(pinned.buf[slot], x + i0 * d, bytes);
			MVS_HIP(hipMemcpyAsync(ws_add.p, pinned.buf[slot], bytes, hipMemcpyHostToDevice, stream));
			pinned.release(slot, stream);
			encode(nb, (const float *)ws_add.p, stream);
			ntotal += nb;
		}
	}
	void add_device(int64_t n, const float *d_x, hipStream_t st) override {
		use_device();
		if (n <= 0)
			return;
		check_add(n);
		store.grow(ntotal + n, ntotal, stream);
		stream_wait(st, stream);
		encode(n, d_x, st);
		stream_wait(stream, st);
		ntotal += n;
	}

	// faiss::IndexFlatCodes::remove_ids: stable compaction of the code rows (csrc/remove_ids.hip); the codebooks stay
	int64_t remove_ids(const mvs_search_params *sel, const int64_t *d_idmap, RemoveMarks *marks) override {
		use_device();
		check_remove_selector(sel);
		if (ntotal <= 0)
			return 0;
		RemoveMarks own;
		RemoveMarks &m = marks ? *marks : own;
		const int64_t nkeep = remove_mark(m, selector.upload(sel, IdDomain::rows(label_offset, ntotal, d_idmap), stream), d_idmap, label_offset, ntotal, stream);
		if (nkeep == ntotal)
			return 0;
		store.compact(m, stream);
		const int64_t removed = ntotal - nkeep;
		ntotal = nkeep;
		return removed;
	}

	// faiss::IndexFlatCodes::merge_from (csrc/merge.hip): M and the codebooks must agree bit for bit; other's code rows follow this store's
	void check_compatible_for_merge(IndexBase &other) override {
		merge_check_common(*this, other);
		PQIndex &o = static_cast<PQIndex &>(other);
		if (M != o.M)
			merge_refuse("M differs (%d against %d)", M, o.M);
		if (!is_trained || !o.is_trained)
			merge_refuse("%s is not trained", is_trained ? "the other index" : "this index");
		use_device();
		stream_wait(stream, o.stream);
		if (!merge_dev_equal(d_cb(), o.d_cb(), cb_floats() * sizeof(float), stream))
			merge_refuse("the PQ codebooks differ");
	}
	void merge_from(IndexBase &other, int64_t add_id) override {
		check_compatible_for_merge(other);
		if (add_id != 0)
			merge_refuse_add_id();
		PQIndex &o = static_cast<PQIndex &>(other);
		use_device();
		MergeLaps laps("PQ");
		const int64_t nb = o.ntotal;
		check_add(nb);
		if (nb > 0) {
			laps.lap("compatibility", stream);
			store.grow(ntotal + nb, ntotal, stream); // (before anything changes: a failure leaves both indexes as they were)
			laps.lap("growth allocation + copy of the old rows", stream);
			stream_wait(stream, o.stream);
			launch_merge_append_rows(o.store.codes(), nullptr, nb, store.pitch, store.codes(), ntotal, stream);
			MVS_HIP(hipStreamSynchronize(stream));
			laps.lap("move kernel", stream);
			ntotal += nb;
		}
		o.ntotal = 0;
		o.store.release();
		laps.lap("the source's reset (its store is freed)", stream);
	}

	// faiss::IndexFlatCodes::reconstruct: sub-vector m is codebook entry code[m] (csrc/reconstruct.hip)
	void recon_source(ReconSource &src, hipStream_t st) override {
		use_device();
		src.mode = RECON_PQ;
		src.rows = store.codes();
		src.pitch = store.pitch;
		src.nrows = ntotal;
		src.cb = d_cb();
		src.M = M, src.dsub = dsub;
		src.push_stage({nullptr, nullptr, (long long)ntotal, (long long)label_offset});
		stream_wait(st, stream);
		src.own(stream);
	}

	// ------------------------------------------------------------------------------------------ search
	struct Chunk { // one chunk of queries: device state of its selection
		int64_t nqc;
		int k, W, G;
		const float *T;
		unsigned long long *bucket, *list;
		int *len, *overflow;
		unsigned *cnt, *thr;
		SelectorDev sel;
		const int64_t *idmap;
		hipStream_t st;
	};
	void launch_scan(const Chunk &c, int64_t r0, int64_t r1, bool timed) {
		const int Q = c.W * c.G;
		const dim3 grid((unsigned)((r1 - r0 + PQ_ROWS_PER_WG - 1) / PQ_ROWS_PER_WG), (unsigned)((c.nqc + Q - 1) / Q));
		const size_t lds = (size_t)Q * M * PQ_KSUB * sizeof(float);
		const int desc = metric == METRIC_IP ? 1 : 0;
		if (timed)
			begin_kernel_timing(c.st);
#define PQ_LAUNCH_SCAN(WW)                                                                                                                          \
	do {                                                                                                                                            \
		ensure_dynamic_lds((const void *)pq_scan_kernel<WW>, lds);                                                                                  \
		hipLaunchKernelGGL(pq_scan_kernel<WW>, grid, dim3(PQ_SCAN_THREADS), lds, c.st, store.codes(), store.pitch, M, (long long)r0, (long long)r1,     \
		                   c.T, c.G, (long long)c.nqc, c.thr, c.bucket, c.cnt, c.overflow, desc, c.sel, (const long long *)c.idmap);                \
	} while (0)
		if (c.W == 4)
			PQ_LAUNCH_SCAN(4);
		else if (c.W == 2)
			PQ_LAUNCH_SCAN(2);
		else
			PQ_LAUNCH_SCAN(1);
#undef PQ_LAUNCH_SCAN
		MVS_HIP(hipGetLastError());
		if (timed) {
			end_kernel_timing(c.st);
			set_kinfo("pq_scan_kernel", (double)c.nqc * (double)(r1 - r0) * M, (double)grid.y * (double)(r1 - r0) * M, (int)(grid.x * grid.y),
			          PQ_SCAN_THREADS, (int)lds, (int)grid.x);
		}
		++last_ranges;
	}
	// rows [r0, r1) into every list of the chunk
	void scan_range(const Chunk &c, int64_t r0, int64_t r1, bool timed) {
		launch_scan(c, r0, r1, timed);
		if (r1 - r0 > PQ_ROWS_PER_WG) { // (a range of at most R rows cannot overflow a bucket of R entries)
			MVS_HIP(hipMemcpyAsync(h_flag.p, c.overflow, sizeof(int), hipMemcpyDeviceToHost, c.st));
			MVS_HIP(hipStreamSynchronize(c.st));
			if (*(const int *)h_flag.p) { // some bucket overflowed: nothing of this range is merged; its two halves one after the other
				MVS_HIP(hipMemsetAsync(c.cnt, 0, (size_t)c.nqc * sizeof(unsigned), c.st));
				MVS_HIP(hipMemsetAsync(c.overflow, 0, sizeof(int), c.st));
				++last_rescans;
				const int64_t mid = r0 + ((r1 - r0) / 2 + PQ_ROWS_PER_WG - 1) / PQ_ROWS_PER_WG * PQ_ROWS_PER_WG;
				scan_range(c, r0, mid, false);
				scan_range(c, mid, r1, false);
				return;
			}
		}
		int P = 1;
		while (P < c.k + PQ_ROWS_PER_WG)
			P <<= 1;
		const size_t lds = (size_t)P * sizeof(unsigned long long);
		ensure_dynamic_lds((const void *)pq_select_kernel, lds);
		hipLaunchKernelGGL(pq_select_kernel, dim3((unsigned)c.nqc), dim3(1024), lds, c.st, c.list, c.len, c.k, c.bucket, c.cnt, c.thr);
		MVS_HIP(hipGetLastError());
	}
	void search_mapped(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, const int64_t *d_idmap,
	                   hipStream_t st) override {
		use_device();
		if (k <= 0)
			throw_faiss("virtual void faiss::Index::search(...) const", "faiss/Index.cpp", "Error: 'k > 0' failed");
		if (k > PQ_MAX_K)
			throw_faiss("mvs::PQIndex::search", __FILE__, "k = %lld is beyond the largest k the PQ index serves on the MI355X path (%d)", (long long)k,
			            PQ_MAX_K);
		if (!is_trained)
			throw_faiss("virtual void faiss::IndexPQ::search(...) const", "faiss/IndexPQ.cpp", "Error: 'is_trained' failed");
		if (nq <= 0)
			return;
		stream_wait(st, stream); // adds were enqueued on our own stream
		const int W = pq_width(M), G = pq_groups(M), Q = W * G;
		// queries per chunk: tables <= 64 MB, buckets <= 256 MB, a multiple of the query block
		int64_t nqc_max = std::min<int64_t>((int64_t)(PQ_TABLE_SCRATCH / ((size_t)M * PQ_KSUB * sizeof(float))),
		                                    (int64_t)(PQ_BUCKET_SCRATCH / ((size_t)PQ_ROWS_PER_WG * sizeof(unsigned long long))));
		nqc_max = std::max<int64_t>(Q, nqc_max / Q * Q);
		nqc_max = std::min<int64_t>(nqc_max, (nq + Q - 1) / Q * Q);
		ws_T.reserve((size_t)nqc_max * M * PQ_KSUB * sizeof(float));
		ws_bucket.reserve((size_t)nqc_max * PQ_ROWS_PER_WG * sizeof(unsigned long long));
		ws_list.reserve((size_t)nqc_max * k * sizeof(unsigned long long));
		// control block: len [nqc] | cnt [nqc] | overflow (+ pad) | thr [nqc]
		const size_t ctl_zero = (size_t)(2 * nqc_max + 4) * sizeof(int);
		ws_ctl.reserve(ctl_zero + (size_t)nqc_max * sizeof(unsigned));
		h_flag.reserve(sizeof(int));
		Chunk c;
		c.k = (int)k, c.W = W, c.G = G;
		c.T = (const float *)ws_T.p;
		c.bucket = (unsigned long long *)ws_bucket.p;
		c.list = (unsigned long long *)ws_list.p;
		c.len = (int *)ws_ctl.p;
		c.cnt = (unsigned *)ws_ctl.p + nqc_max;
		c.overflow = (int *)ws_ctl.p + 2 * nqc_max;
		c.thr = (unsigned *)((char *)ws_ctl.p + ctl_zero);
		c.sel = selector.upload(params, IdDomain::rows(0, ntotal, d_idmap), st); // (the scan tests d_idmap[row], or the row)
		c.idmap = d_idmap;
		c.st = st;
		last_ranges = last_rescans = 0;
		for (int64_t q0 = 0; q0 < nq; q0 += nqc_max) {
			c.nqc = std::min(nqc_max, nq - q0);
			MVS_HIP(hipMemsetAsync(ws_ctl.p, 0, ctl_zero, st));
			pq_open_bounds(c.thr, (size_t)nqc_max, st); // (an open list admits what FAISS's neutral-filled heap admits: csrc/pq_kernels.h)
			hipLaunchKernelGGL(pq_tables_kernel, dim3((unsigned)c.nqc, (unsigned)M), dim3(PQ_KSUB), 0, st, d_x + q0 * d, d, M, dsub, d_cb(),
			                   metric == METRIC_L2 ? 1 : 0, W, G, (float *)ws_T.p);
			MVS_HIP(hipGetLastError());
			for (int64_t r0 = 0, r1 = std::min<int64_t>(ntotal, PQ_ROWS_PER_WG); r0 < ntotal; r0 = r1, r1 = std::min(ntotal, 3 * r1))
				scan_range(c, r0, r1, r1 == ntotal);
			const int64_t tot = c.nqc * k;
			hipLaunchKernelGGL(pq_emit_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, c.list, c.len, c.k, (long long)c.nqc,
			                   metric == METRIC_IP ? 1 : 0, raw_labels ? nullptr : (const long long *)d_idmap, (long long)label_offset, d_D + q0 * k, // (raw_labels: csrc/index.h)
			                   (long long *)(d_I + q0 * k));
			MVS_HIP(hipGetLastError());
		}
	}
	void search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, hipStream_t st) override {
		search_mapped(nq, d_x, k, d_D, d_I, params, nullptr, st);
	}
	bool named_stat(const char *name, int64_t *value) override {
		if (!strcmp(name, "pq_query_block"))
			*value = pq_width(M) * pq_groups(M);
		else if (!strcmp(name, "pq_rows_per_workgroup"))
			*value = PQ_ROWS_PER_WG;
		else if (!strcmp(name, "pq_scan_launches"))
			*value = last_ranges;
		else if (!strcmp(name, "pq_scan_rescans"))
			*value = last_rescans;
		else
			return false;
		return true;
	}
	size_t device_bytes() const override {
		return (size_t)store.cap * store.pitch + (d_cb() ? cb_floats() * sizeof(float) : 0);
	}

	// ------------------------------------------------------------------------------------------ images, placement
	void get_centroids(float *out) {
		use_device();
		if (!d_cb())
			throw_faiss("mvs::PQIndex::get_centroids", __FILE__, "the index is not trained");
		MVS_HIP(hipStreamSynchronize(stream));
		MVS_HIP(hipMemcpy(out, d_cb(), cb_floats() * sizeof(float), hipMemcpyDeviceToHost));
	}
	void get_codes(int64_t row0, int64_t n, uint8_t *out) {
		use_device();
		if (row0 < 0 || n < 0 || row0 + n > ntotal)
			throw_faiss("mvs::PQIndex::get_codes", __FILE__, "rows [%lld, %lld) are outside the index (ntotal %lld)", (long long)row0,
			            (long long)(row0 + n), (long long)ntotal);
		MVS_HIP(hipStreamSynchronize(stream));
		if (n > 0)
			MVS_HIP(hipMemcpy2D(out, (size_t)M, store.codes() + (size_t)row0 * store.pitch, (size_t)store.pitch, (size_t)M, (size_t)n, hipMemcpyDeviceToHost));
	}
	void to_host(HostIndex &out) override {
		out.kind = MVS_KIND_PQ;
		out.d = d;
		out.metric = metric;
		out.metric_arg = metric_arg;
		out.ntotal = ntotal;
		out.is_trained = is_trained;
		out.pq_M = M;
		out.pq_centroids.assign(cb_floats(), 0.f); // (FAISS allocates the codebooks with the ProductQuantizer: an untrained image holds zeros)
		if (is_trained)
			get_centroids(out.pq_centroids.data());
		out.pq_codes.resize((size_t)ntotal * M);
		get_codes(0, ntotal, out.pq_codes.data());
	}
	void load_image(const HostIndex &h) { // an empty index on its device <- codebooks and codes of the image
		if (h.pq_centroids.size() != cb_floats() || (int64_t)h.pq_codes.size() != h.ntotal * M)
			throw_faiss("faiss::Index* faiss::read_index(...)", "faiss/impl/index_read.cpp", "PQ image: %zu centroid values and %zu code bytes do not "
			            "match d = %d, M = %d, ntotal = %lld", h.pq_centroids.size(), h.pq_codes.size(), d, M, (long long)h.ntotal);
		if (h.ntotal > (int64_t)0x7fffffff - 1024)
			throw_faiss("mvs::PQIndex::add", __FILE__, "a single-device index holds at most 2^31 rows");
		use_device();
		metric_arg = h.metric_arg;
		if (h.is_trained)
			set_centroids(h.pq_centroids.data());
		store.grow(h.ntotal, ntotal, stream);
		if (h.ntotal > 0)
			MVS_HIP(hipMemcpy2D(store.codes(), (size_t)store.pitch, h.pq_codes.data(), (size_t)M, (size_t)M, (size_t)h.ntotal, hipMemcpyHostToDevice));
		ntotal = h.ntotal;
	}
	void to_device(int new_device) override {
		if (new_device == device)
			return;
		check_device(new_device);
		HostIndex img;
		to_host(img);
		use_device();
		MVS_HIP(hipStreamSynchronize(stream));
		free_device();
		move_stream(new_device);
		ntotal = 0;
		load_image(img);
	}
	IndexBase *clone(int on_device) override {
		HostIndex img;
		to_host(img);
		IndexBase *c = pq_from_host(img, on_device);
		c->label_offset = label_offset;
		return c;
	}
};

} // namespace

// "PQ<M>" | "PQ<M>x8" (faiss/index_factory.cpp); nullptr if desc is not a PQ string
IndexBase *make_pq_index(int d, const std::string &desc, int metric) {
	if (desc.rfind("PQ", 0) != 0)
		return nullptr;
	char *end = nullptr;
	const long M = strtol(desc.c_str() + 2, &end, 10);
	if (end == desc.c_str() + 2 || M <= 0)
		return nullptr;
	const char *fn = "faiss::Index* faiss::index_factory(int, const char*, faiss::MetricType)";
	if (*end) { // "x<nbits>": 8 only; anything else (PQ<M>np, PQ<M>x<b>fs, ...) is a variant this path does not have
		char *end2 = nullptr;
		const long nbits = *end == 'x' ? strtol(end + 1, &end2, 10) : 0;
		if (*end != 'x' || end2 == end + 1 || *end2 || nbits != 8)
			throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s (8 bits per code only)",
			            desc.c_str());
	}
	if (M > PQ_MAX_M)
		throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s (at most %d subquantizers)",
		            desc.c_str(), PQ_MAX_M);
	if (d % M != 0)
		throw_faiss("faiss::ProductQuantizer::set_derived_values()", "faiss/impl/ProductQuantizer.cpp",
		            "Error: 'd %% M == 0' failed: The dimension of the vector (d) should be a multiple of the number of subquantizers (M)");
	return new PQIndex(d, (int)M, metric);
}
IndexBase *pq_from_host(const HostIndex &h, int device) {
	CtorDevice scope(device);
	if (h.pq_M <= 0 || h.pq_M > PQ_MAX_M || h.d % h.pq_M != 0)
		throw_faiss("faiss::Index* faiss::read_index(...)", "faiss/impl/index_read.cpp", "PQ image with M = %d at d = %d is not served on the MI355X path",
		            h.pq_M, h.d);
	auto *p = new PQIndex(h.d, h.pq_M, h.metric);
	try {
		p->load_image(h);
	} catch (...) {
		delete p;
		throw;
	}
	return p;
}
bool pq_info(const IndexBase *ix, int *M, int *nbits) {
	if (ix->kind == MVS_KIND_IVFPQ)
		return ivfpq_info(ix, M, nbits);
	if (ix->kind != MVS_KIND_PQ)
		return false;
	if (M)
		*M = static_cast<const PQIndex *>(ix)->M;
	if (nbits)
		*nbits = 8;
	return true;
}
bool pq_get_centroids(IndexBase *ix, float *out) {
	if (ix->kind == MVS_KIND_IVFPQ)
		return ivfpq_get_codebooks(ix, out);
	if (ix->kind != MVS_KIND_PQ)
		return false;
	static_cast<PQIndex *>(ix)->get_centroids(out);
	return true;
}
bool pq_set_centroids(IndexBase *ix, const float *c) {
	if (ix->kind == MVS_KIND_IVFPQ) // (trained once the coarse centroids are present too)
		return ivfpq_set_codebooks(ix, c);
	if (ix->kind != MVS_KIND_PQ)
		return false;
	static_cast<PQIndex *>(ix)->set_centroids(c);
	return true;
}
bool pq_get_codes(IndexBase *ix, int64_t row0, int64_t n, uint8_t *out) {
	if (ix->kind != MVS_KIND_PQ)
		return false;
	static_cast<PQIndex *>(ix)->get_codes(row0, n, out);
	return true;
}

} // namespace mvs
