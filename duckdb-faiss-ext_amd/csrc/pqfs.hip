// csrc/pqfs.hip -- 4-bit product-quantised index "PQ<M>x4fs" (faiss::IndexPQFastScan), scanned on the int8 matrix pipe.
//
// Contract (include/mi355_faiss.h "4-bit product-quantised indexes"):
//   train   codebook m = the 16 centroids IVF16,Flat (L2) learns from columns [m dsub, (m+1) dsub)
//   encode  PQ's rule over 16 entries: argmin_j of acc = fmaf(t, t, acc), t = x[k] - c[k]; smallest j on a tie
//   search  per query: T[m][j] = PQ's f32 chain; lo_m / hi_m = min / max over j; span = max_m (hi_m - lo_m); a = 255 / span (0 if span == 0);
//           b = ((lo_0 + lo_1) + ...); tq[m][j] = clamp((int)floorf(fmaf(T[m][j] - lo_m, a, 0.5f)), 0, 255).  A row's score is the exact integer
//           s = sum_m tq[m][code_m]; the order is total on (s, row); the distance printed is b + (float)s / a (b when a == 0)
//
// A row's score is the dot product of the query's M x 16 table bytes with the row's one-hot expansion: an int8 GEMM with K = 16 M.  One
// v_mfma_i32_16x16x64_i8 covers 4 sub-quantisers (its four K-groups of 16 slots) for 16 queries x 16 rows.
//
// Kernels
//   pqfs_encode_kernel  one lane per (row, K-group, chunk of 8 steps): its 8 nibbles, one dword out, in the store's layout
//   pqfs_tables_kernel  one workgroup per query: T in LDS, lo / hi / span, a, b, then the bytes tq - 128 (the MFMA's operands are signed)
//                       in the scan's A-fragment order; M padded to a multiple of 4 with zero bytes; (a, b, non-finite flag) per query
//   pqfs_scan_kernel<T, SMAX>  the hot path, query-stationary: a wave keeps the A fragments of T 16-query tiles in registers (4 SMAX VGPRs
//                       a tile), the four waves of a workgroup walk different 16-row tiles of the workgroup's PQ_ROWS_PER_WG rows.  Per row
//                       tile and step a lane expands its nibble into the 16-byte one-hot B operand, which serves all T query tiles.  No LDS
//                       in the row walk.  i32 sums; a sum that beats its query's bound goes to the query's bucket (csrc/pq.hip's stream)
//   pq_select_kernel    csrc/pq_kernels.h, on 32-bit keys made from s
//   pqfs_emit_kernel    keys -> b + s / a and labels (IDMap: id_map[row]), -1 / +-FLT_MAX padded
//   pqfs_unpack_kernel / pqfs_pack_kernel  the store <-> FAISS's packing (code of even m in the low nibble of byte m / 2)
//   (decode: csrc/reconstruct.hip RECON_PQ4)
//
// Code store.  Tiles of 16 rows; a tile is `chunks` = ceil(M / 32) planes of 64 dwords.  Dword l of plane c belongs to the lane l of the
// scan: row l & 15 of the tile, K-group g = l >> 4; its nibble t is the code of sub-quantiser m = 4 (8 c + t) + g -- the lane's operand
// of step 8 c + t.  One coalesced 256-byte load per plane feeds 8 steps.  (pqfs_code_word / pqfs_code_shift, csrc/index.h)
#include "coded_lists.h"
#include "pq_kernels.h"
#include "pqfs_kernels.h"

#include <cfloat>
#include <climits>
#include <cstring>

namespace mvs {

namespace {

constexpr unsigned PQFS_KEY_TOP = 0xFFFFu;      // s <= 255 * 128 = 32640; inner product: key = PQFS_KEY_TOP - s
constexpr unsigned PQFS_OPEN_BOUND = 0x10000u;  // above every key: an open list admits every row
constexpr int PQFS_SCAN_THREADS = 256;          // four waves, one per SIMD

// ---------------------------------------------------------------------------------------------- encode, pack, unpack
// rows x [n][d] -> rows [row0, row0 + n) of the store
__global__ __launch_bounds__(256) void pqfs_encode_kernel(const float *__restrict__ x, long long n, int d, int M, int dsub, const float *__restrict__ cb,
                                                          unsigned *__restrict__ codes, int chunks, long long row0) {
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	const long long r = i / (4 * chunks);
	if (r >= n)
		return;
	const int cg = (int)(i - r * 4 * chunks), c = cg >> 2, g = cg & 3;
	unsigned w = 0;
	for (int t = 0; t < 8; ++t) {
		const int m = 32 * c + 4 * t + g;
		if (m >= M)
			break;
		const float *xv = x + r * d + (long long)m * dsub;
		float best = 0.f;
		unsigned bj = 0;
		for (int j = 0; j < PQFS_KSUB; ++j) {
			const float acc = pqfs_chain(xv, cb + ((size_t)m * PQFS_KSUB + j) * dsub, dsub, 1);
			if (j == 0 || acc < best) {
				best = acc;
				bj = (unsigned)j;
			}
		}
		w |= bj << (4 * t);
	}
	codes[pqfs_code_word(row0 + r, 32 * c + g, chunks)] = w;
}
// FAISS's packing in [n][M / 2] -> rows [row0, row0 + n) of the store
__global__ __launch_bounds__(256) void pqfs_pack_kernel(const unsigned char *__restrict__ in, long long n, int M, unsigned *__restrict__ codes, int chunks,
                                                        long long row0) {
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	const long long r = i / (4 * chunks);
	if (r >= n)
		return;
	const int cg = (int)(i - r * 4 * chunks), c = cg >> 2, g = cg & 3;
	unsigned w = 0;
	for (int t = 0; t < 8; ++t) {
		const int m = 32 * c + 4 * t + g;
		if (m < M)
			w |= (unsigned)((in[r * (M / 2) + (m >> 1)] >> ((m & 1) * 4)) & 15) << (4 * t);
	}
	codes[pqfs_code_word(row0 + r, 32 * c + g, chunks)] = w;
}
// rows [row0, row0 + n) of the store -> FAISS's packing
__global__ __launch_bounds__(256) void pqfs_unpack_kernel(const unsigned *__restrict__ codes, int chunks, long long row0, long long n, int M,
                                                          unsigned char *__restrict__ out) {
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	const int hb = M / 2;
	const long long r = i / hb;
	if (r >= n)
		return;
	const int m = 2 * (int)(i - r * hb);
	const unsigned lo = (codes[pqfs_code_word(row0 + r, m, chunks)] >> pqfs_code_shift(m)) & 15u;
	const unsigned hi = (codes[pqfs_code_word(row0 + r, m + 1, chunks)] >> pqfs_code_shift(m + 1)) & 15u;
	out[i] = (unsigned char)(lo | (hi << 4));
}

// ---------------------------------------------------------------------------------------------- tables
// A [query tile][step][lane]: 16 bytes, the lane's operand -- query l & 15 of the tile, sub-quantiser 4 step + (l >> 4), byte j = tq[m][j] - 128.
// The grid covers whole query blocks: a query past the chunk's end gets zero bytes
__global__ __launch_bounds__(256) void pqfs_tables_kernel(const float *__restrict__ xq, long long nqc, int d, int M, int dsub, const float *__restrict__ cb,
                                                          int is_l2, int S, pqfs_i32x4 *__restrict__ A, float *__restrict__ qa, float *__restrict__ qb,
                                                          int *__restrict__ qflag) {
	__shared__ float T[PQFS_MAX_M * PQFS_KSUB];
	__shared__ float lo[PQFS_MAX_M], hi[PQFS_MAX_M];
	__shared__ float s_a;
	__shared__ int s_bad;
	const long long q = blockIdx.x;
	const int tid = threadIdx.x;
	pqfs_i32x4 *Aq = A + (q >> 4) * S * 64 + (q & 15);
	if (q >= nqc) {
		for (int m = tid; m < 4 * S; m += 256)
			Aq[(m >> 2) * 64 + (m & 3) * 16] = pqfs_i32x4 {0, 0, 0, 0};
		return;
	}
	if (tid == 0)
		s_bad = 0;
	__syncthreads();
	for (int e = tid; e < M * PQFS_KSUB; e += 256) {
		const int m = e >> 4;
		const float v = pqfs_chain(xq + q * d + (long long)m * dsub, cb + (size_t)e * dsub, dsub, is_l2);
		T[e] = v;
		if (!(fabsf(v) <= FLT_MAX)) // NaN or inf
			s_bad = 1;
	}
	__syncthreads();
	if (tid < M) {
		float l = T[tid * PQFS_KSUB], h = l;
		for (int j = 1; j < PQFS_KSUB; ++j) {
			l = fminf(l, T[tid * PQFS_KSUB + j]);
			h = fmaxf(h, T[tid * PQFS_KSUB + j]);
		}
		lo[tid] = l, hi[tid] = h;
	}
	__syncthreads();
	if (tid == 0) {
		float span = 0.f, b = 0.f;
		for (int m = 0; m < M; ++m) {
			span = fmaxf(span, __fsub_rn(hi[m], lo[m]));
			b = m == 0 ? lo[0] : __fadd_rn(b, lo[m]);
		}
		const float a = s_bad || span == 0.f ? 0.f : __fdiv_rn(255.f, span);
		qa[q] = a, qb[q] = b, qflag[q] = s_bad;
		s_a = a;
	}
	__syncthreads();
	const float a = s_a;
	for (int m = tid; m < 4 * S; m += 256) {
		Aq[(m >> 2) * 64 + (m & 3) * 16] = m < M ? pqfs_quantise16(T + m * PQFS_KSUB, lo[m], a) : pqfs_i32x4 {0, 0, 0, 0};
	}
}

// ---------------------------------------------------------------------------------------------- scan
// rows [r0, r1) against the T 16-query tiles of block blockIdx.y; workgroup blockIdx.x walks rows r0 + blockIdx.x R ... (+ R), r0 a multiple
// of 16.  SMAX: the steps the instance unrolls, a power of two >= S = ceil(M / 4); a step past S has zero A fragments and zero code planes.
// T SMAX <= 64: 256 of a lane's 512 registers hold A fragments -- one wave per SIMD
template <int T, int SMAX>
__global__ __launch_bounds__(PQFS_SCAN_THREADS) void pqfs_scan_kernel(const unsigned *__restrict__ codes, int chunks, int S, int M, long long r0, long long r1,
                                                                      const pqfs_i32x4 *__restrict__ A, long long nqc, const unsigned *__restrict__ thr,
                                                                      const int *__restrict__ qflag, unsigned long long *__restrict__ bucket,
                                                                      unsigned *__restrict__ cnt, int *__restrict__ overflow, int descending, SelectorDev sel,
                                                                      const long long *__restrict__ idmap) {
	constexpr int CH = SMAX > 8 ? SMAX / 8 : 1; // code planes a tile has at most
	constexpr int UT = 2;                       // row tiles in flight per wave
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const long long qt0 = (long long)blockIdx.y * T; // the block's first query tile
	pqfs_i32x4 a[T][SMAX];
#pragma unroll
	for (int t = 0; t < T; ++t)
#pragma unroll
		for (int st = 0; st < SMAX; ++st)
			a[t][st] = st < S ? A[((qt0 + t) * S + st) * 64 + lane] : pqfs_i32x4 {0, 0, 0, 0};
	// the bounds on the accumulator's side: acc (L2) / -acc (inner product) enters below bnd; INT_MIN admits nothing
	int bnd[T][4];
	const int bias = 128 * M;
#pragma unroll
	for (int t = 0; t < T; ++t)
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const long long q = (qt0 + t) * 16 + 4 * (lane >> 4) + i;
			bnd[t][i] = INT_MIN;
			if (q < nqc && !qflag[q])
				bnd[t][i] = descending ? (int)thr[q] - (int)PQFS_KEY_TOP + bias : (int)thr[q] - bias;
		}
	const long long wg0 = r0 + (long long)blockIdx.x * PQ_ROWS_PER_WG;
	const long long wg1 = wg0 + PQ_ROWS_PER_WG < r1 ? wg0 + PQ_ROWS_PER_WG : r1;
	const long long tile0 = wg0 >> 4;
	const int ntile = (int)((wg1 - wg0 + 15) >> 4);
	unsigned cur[UT][CH], nxt[UT][CH];
#pragma unroll
	for (int u = 0; u < UT; ++u)
#pragma unroll
		for (int c = 0; c < CH; ++c)
			cur[u][c] = wave + 4 * u < ntile && c < chunks ? codes[((tile0 + wave + 4 * u) * chunks + c) * 64 + lane] : 0u;
	for (int tl = wave; tl < ntile; tl += 4 * UT) {
#pragma unroll
		for (int u = 0; u < UT; ++u)
#pragma unroll
			for (int c = 0; c < CH; ++c) {
				const int tn = tl + 4 * (UT + u);
				nxt[u][c] = tn < ntile && c < chunks ? codes[((tile0 + tn) * chunks + c) * 64 + lane] : 0u;
			}
#pragma unroll
		for (int u = 0; u < UT; ++u) {
			if (tl + 4 * u >= ntile)
				break;
			pqfs_i32x4 acc[T];
#pragma unroll
			for (int t = 0; t < T; ++t)
				acc[t] = pqfs_i32x4 {0, 0, 0, 0};
#pragma unroll
			for (int st = 0; st < SMAX; ++st) {
				const pqfs_i32x4 b = pqfs_one_hot((cur[u][st >> 3] >> ((st & 7) * 4)) & 15u);
#pragma unroll
				for (int t = 0; t < T; ++t)
					acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t][st], b, acc[t], 0, 0, 0);
			}
			// acc[t][i]: query 4 (lane >> 4) + i of tile t against row lane & 15 of the row tile
			bool any = false;
#pragma unroll
			for (int t = 0; t < T; ++t)
#pragma unroll
				for (int i = 0; i < 4; ++i)
					any |= (descending ? -acc[t][i] : acc[t][i]) < bnd[t][i];
			const long long row = ((tile0 + tl + 4 * u) << 4) + (lane & 15);
			if (any && row < wg1 && (sel.kind == MVS_SEL_NONE || pq_sel_member(sel, idmap ? idmap[row] : row))) {
#pragma unroll
				for (int t = 0; t < T; ++t)
#pragma unroll
					for (int i = 0; i < 4; ++i)
						if ((descending ? -acc[t][i] : acc[t][i]) < bnd[t][i]) {
							const long long q = (qt0 + t) * 16 + 4 * (lane >> 4) + i;
							const unsigned s = (unsigned)(acc[t][i] + bias);
							const unsigned key = descending ? PQFS_KEY_TOP - s : s;
							const unsigned pos = atomicAdd(&cnt[q], 1u);
							if (pos < (unsigned)PQ_ROWS_PER_WG)
								bucket[(size_t)q * PQ_ROWS_PER_WG + pos] = ((unsigned long long)key << 32) | (unsigned long long)(unsigned)row;
							else
								*overflow = 1;
						}
			}
		}
#pragma unroll
		for (int u = 0; u < UT; ++u)
#pragma unroll
			for (int c = 0; c < CH; ++c)
				cur[u][c] = nxt[u][c];
	}
}

// ---------------------------------------------------------------------------------------------- emit
__global__ __launch_bounds__(256) void pqfs_emit_kernel(const unsigned long long *__restrict__ list, const int *__restrict__ len, int k, long long nqc,
                                                        int descending, const float *__restrict__ qa, const float *__restrict__ qb,
                                                        const long long *__restrict__ idmap, long long label_offset, float *__restrict__ D,
                                                        long long *__restrict__ I) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nqc * k)
		return;
	const long long q = i / k;
	const int slot = (int)(i - q * k);
	if (slot < len[q]) {
		const unsigned long long e = list[i];
		const long long row = (long long)(e & 0xFFFFFFFFull);
		const unsigned key = (unsigned)(e >> 32);
		const float s = (float)(descending ? PQFS_KEY_TOP - key : key), a = qa[q];
		D[i] = a == 0.f ? qb[q] : __fadd_rn(qb[q], __fdiv_rn(s, a));
		I[i] = idmap ? idmap[row] : row + label_offset;
	} else {
		D[i] = descending ? -FLT_MAX : FLT_MAX;
		I[i] = -1;
	}
}

// ---------------------------------------------------------------------------------------------- index
struct PQFSWork { // every device workspace a PQFSIndex keeps between calls (as PQWork, csrc/pq.hip)
	DevBuf ws_add, ws_A, ws_q, ws_bucket, ws_list, ws_ctl, ws_pack;
	void release_all() {
		DevBuf *const all[] = {&ws_add, &ws_A, &ws_q, &ws_bucket, &ws_list, &ws_ctl, &ws_pack};
		static_assert(sizeof all / sizeof *all * sizeof(DevBuf) == sizeof(PQFSWork), "a workspace of PQFSWork is missing from release_all()");
		for (DevBuf *b : all)
			b->release();
	}
};

[[noreturn]] void pqfs_refuse(const char *fn, const char *file, const char *what) {
	throw_faiss(fn, file, "This index type is not implemented on the MI355X path yet: %s over PQ<M>x4fs", what);
}

class PQFSIndex : public IndexBase, public PQFSWork {
public:
	const int M, dsub, S, chunks; // S = ceil(M / 4) MFMA steps; chunks = ceil(M / 32) code planes per row tile
	DevBlock<float> cb_;          // [M][16][dsub]; null until set_centroids
	CodeStore store;              // 16 chunks bytes a row; a tile of 16 rows is contiguous, so rows are kept and grown in whole tiles
	PinnedMem h_flag;
	SelectorHolder selector;
	int64_t last_ranges = 0, last_rescans = 0;

	PQFSIndex(int d_, int M_, int metric_)
	    : IndexBase(MVS_KIND_PQFS, d_, metric_), M(M_), dsub(d_ / M_), S((M_ + 3) / 4), chunks((M_ + 31) / 32), store(16 * ((M_ + 31) / 32)) {
		if (metric != METRIC_L2 && metric != METRIC_IP)
			throw_faiss("mvs::PQFSIndex", __FILE__, "metric type %d is not implemented on the MI355X path", metric);
		is_trained = false;
	}
	~PQFSIndex() override {
		(void)hipSetDevice(device);
		if (stream)
			(void)hipStreamSynchronize(stream);
	}
	float *d_cb() const {
		return cb_.get();
	}
	unsigned *d_codes() const {
		return (unsigned *)store.codes();
	}
	size_t cb_floats() const {
		return (size_t)M * PQFS_KSUB * dsub;
	}
	static int64_t tiles16(int64_t rows) {
		return (rows + 15) / 16 * 16;
	}

	// ------------------------------------------------------------------------------------------ train
	void check_empty_for_training() const {
		if (ntotal > 0)
			throw_faiss("mvs::PQFSIndex::train", __FILE__, "the index already holds %lld rows encoded with its codebooks: training again is "
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
	void train(int64_t n, const float *x) override { // one Clustering(dsub, 16) per sub-space, L2, 10 iterations (as csrc/pq.hip)
		use_device();
		check_empty_for_training();
		std::vector<float> cent(cb_floats()), cols((size_t)std::max<int64_t>(n, 0) * dsub);
		for (int m = 0; m < M; ++m) {
			for (int64_t i = 0; i < n; ++i)
				memcpy(&cols[(size_t)i * dsub], x + i * d + (int64_t)m * dsub, (size_t)dsub * sizeof(float));
			CtorDevice scope(device);
			FlatIndex assigner(dsub, METRIC_L2);
			assigner.adopt_tuning(tune_);
			kmeans_train({PQFS_KSUB, 10, false}, n, cols.data(), assigner);
			assigner.copy_rows_to_host(&cent[(size_t)m * PQFS_KSUB * dsub]);
		}
		set_centroids(cent.data());
	}

	// ------------------------------------------------------------------------------------------ add
	void check_add(int64_t n) {
		if (!is_trained)
			throw_faiss("virtual void faiss::IndexFastScan::add(...)", "faiss/IndexFastScan.cpp", "Error: 'is_trained' failed");
		if (ntotal + n > (int64_t)0x7fffffff - 1024)
			throw_faiss("mvs::PQFSIndex::add", __FILE__, "a single-device index holds at most 2^31 rows");
	}
	void grow(int64_t n) {
		store.grow(tiles16(ntotal + n), tiles16(ntotal), stream);
	}
	unsigned lane_grid(int64_t n) const { // one lane per (row, K-group, plane)
		return (unsigned)((n * 4 * chunks + 255) / 256);
	}
	void encode(int64_t n, const float *d_x, hipStream_t st) {
		hipLaunchKernelGGL(pqfs_encode_kernel, dim3(lane_grid(n)), dim3(256), 0, st, d_x, (long long)n, d, M, dsub, d_cb(), d_codes(), chunks, (long long)ntotal);
		MVS_HIP(hipGetLastError());
	}
	void add(int64_t n, const float *x) override {
		use_device();
		if (n <= 0)
			return;
		check_add(n);
		grow(n);
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
		grow(n);
		stream_wait(st, stream);
		encode(n, d_x, st);
		stream_wait(stream, st);
		ntotal += n;
	}

	// ------------------------------------------------------------------------------------------ what the kind does not serve yet
	void range_search(int64_t, const float *, float, const mvs_search_params *, RangeResult &) override {
		pqfs_refuse("virtual void faiss::Index::range_search(...) const", "faiss/Index.cpp", "range_search");
	}
	void range_search_mapped(int64_t, const float *, float, const mvs_search_params *, const int64_t *, RangeResult &, hipStream_t) override {
		pqfs_refuse("virtual void faiss::Index::range_search(...) const", "faiss/Index.cpp", "range_search");
	}
	int64_t remove_ids(const mvs_search_params *, const int64_t *, RemoveMarks *) override {
		pqfs_refuse("virtual size_t faiss::Index::remove_ids(const faiss::IDSelector&)", "faiss/Index.cpp", "remove_ids");
	}
	void check_compatible_for_merge(IndexBase &) override {
		pqfs_refuse("virtual void faiss::Index::check_compatible_for_merge(const faiss::Index&) const", "faiss/Index.cpp", "merge_from");
	}
	void merge_from(IndexBase &, int64_t) override {
		pqfs_refuse("virtual void faiss::Index::merge_from(faiss::Index&, faiss::idx_t)", "faiss/Index.cpp", "merge_from");
	}

	// sub-vector m of a row is codebook entry code[m] (csrc/reconstruct.hip RECON_PQ4)
	void recon_source(ReconSource &src, hipStream_t st) override {
		use_device();
		src.mode = RECON_PQ4;
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
	struct Chunk {
		int64_t nqc;
		int k;
		const pqfs_i32x4 *A;
		const float *qa, *qb;
		const int *qflag;
		unsigned long long *bucket, *list;
		int *len, *overflow;
		unsigned *cnt, *thr;
		SelectorDev sel;
		const int64_t *idmap;
		hipStream_t st;
	};
	// the instance: SMAX the power of two that holds S steps, T SMAX = 64
	int smax() const {
		int s = 2;
		while (s < S)
			s <<= 1;
		return s;
	}
	int query_tiles() const {
		return std::min(8, 64 / smax());
	}
	void launch_scan(const Chunk &c, int64_t r0, int64_t r1, bool timed) {
		const int T = query_tiles();
		const dim3 grid((unsigned)((r1 - r0 + PQ_ROWS_PER_WG - 1) / PQ_ROWS_PER_WG), (unsigned)((c.nqc + 16 * T - 1) / (16 * T)));
		const int desc = metric == METRIC_IP ? 1 : 0;
		if (timed)
			begin_kernel_timing(c.st);
#define PQFS_LAUNCH_SCAN(TT, SS)                                                                                                                     \
	hipLaunchKernelGGL((pqfs_scan_kernel<TT, SS>), grid, dim3(PQFS_SCAN_THREADS), 0, c.st, (const unsigned *)d_codes(), chunks, S, M, (long long)r0, \
	                   (long long)r1, c.A, (long long)c.nqc, c.thr, c.qflag, c.bucket, c.cnt, c.overflow, desc, c.sel, (const long long *)c.idmap)
		switch (smax()) {
		case 2:
			PQFS_LAUNCH_SCAN(8, 2);
			break;
		case 4:
			PQFS_LAUNCH_SCAN(8, 4);
			break;
		case 8:
			PQFS_LAUNCH_SCAN(8, 8);
			break;
		case 16:
			PQFS_LAUNCH_SCAN(4, 16);
			break;
		default:
			PQFS_LAUNCH_SCAN(2, 32);
			break;
		}
#undef PQFS_LAUNCH_SCAN
		MVS_HIP(hipGetLastError());
		if (timed) {
			end_kernel_timing(c.st);
			// 2 K ops per (query, row) of the padded GEMM, K = 16 slots a sub-quantiser; bytes: every query block reads the range's code planes
			set_kinfo("pqfs_scan_kernel", 2.0 * 16.0 * 4.0 * S * (double)(grid.y * 16 * T) * (double)(r1 - r0), (double)grid.y * (double)(r1 - r0) * store.pitch,
			          (int)(grid.x * grid.y), PQFS_SCAN_THREADS, 0, (int)grid.x);
		}
		++last_ranges;
	}
	void scan_range(const Chunk &c, int64_t r0, int64_t r1, bool timed) { // rows [r0, r1) into every list of the chunk (as csrc/pq.hip)
		launch_scan(c, r0, r1, timed);
		if (r1 - r0 > PQ_ROWS_PER_WG) {
			MVS_HIP(hipMemcpyAsync(h_flag.p, c.overflow, sizeof(int), hipMemcpyDeviceToHost, c.st));
			MVS_HIP(hipStreamSynchronize(c.st));
			if (*(const int *)h_flag.p) {
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
			throw_faiss("mvs::PQFSIndex::search", __FILE__, "k = %lld is beyond the largest k the PQ index serves on the MI355X path (%d)", (long long)k,
			            PQ_MAX_K);
		if (!is_trained)
			throw_faiss("virtual void faiss::IndexFastScan::search(...) const", "faiss/IndexFastScan.cpp", "Error: 'is_trained' failed");
		if (nq <= 0)
			return;
		stream_wait(st, stream);
		const int Q = 16 * query_tiles();
		int64_t nqc_max = (int64_t)(PQ_BUCKET_SCRATCH / ((size_t)PQ_ROWS_PER_WG * sizeof(unsigned long long))); // buckets <= 256 MB
		nqc_max = std::min<int64_t>(nqc_max / Q * Q, (nq + Q - 1) / Q * Q);
		ws_A.reserve((size_t)nqc_max * S * 4 * sizeof(pqfs_i32x4));
		ws_q.reserve((size_t)nqc_max * 3 * sizeof(float));
		ws_bucket.reserve((size_t)nqc_max * PQ_ROWS_PER_WG * sizeof(unsigned long long));
		ws_list.reserve((size_t)nqc_max * k * sizeof(unsigned long long));
		// control block: len [nqc] | cnt [nqc] | overflow (+ pad) | thr [nqc]
		const size_t ctl_zero = (size_t)(2 * nqc_max + 4) * sizeof(int);
		ws_ctl.reserve(ctl_zero + (size_t)nqc_max * sizeof(unsigned));
		h_flag.reserve(sizeof(int));
		Chunk c;
		c.k = (int)k;
		c.A = (const pqfs_i32x4 *)ws_A.p;
		c.qa = (const float *)ws_q.p, c.qb = c.qa + nqc_max, c.qflag = (const int *)(c.qb + nqc_max);
		c.bucket = (unsigned long long *)ws_bucket.p;
		c.list = (unsigned long long *)ws_list.p;
		c.len = (int *)ws_ctl.p;
		c.cnt = (unsigned *)ws_ctl.p + nqc_max;
		c.overflow = (int *)ws_ctl.p + 2 * nqc_max;
		c.thr = (unsigned *)((char *)ws_ctl.p + ctl_zero);
		c.sel = selector.upload(params, IdDomain::rows(0, ntotal, d_idmap), st);
		c.idmap = d_idmap;
		c.st = st;
		last_ranges = last_rescans = 0;
		for (int64_t q0 = 0; q0 < nq; q0 += nqc_max) {
			c.nqc = std::min(nqc_max, nq - q0);
			MVS_HIP(hipMemsetAsync(ws_ctl.p, 0, ctl_zero, st));
			MVS_HIP(hipMemsetD32Async((hipDeviceptr_t)c.thr, (int)PQFS_OPEN_BOUND, (size_t)nqc_max, st));
			hipLaunchKernelGGL(pqfs_tables_kernel, dim3((unsigned)((c.nqc + Q - 1) / Q * Q)), dim3(256), 0, st, d_x + q0 * d, (long long)c.nqc, d, M, dsub, d_cb(),
			                   metric == METRIC_L2 ? 1 : 0, S, (pqfs_i32x4 *)ws_A.p, (float *)c.qa, (float *)c.qb, (int *)c.qflag);
			MVS_HIP(hipGetLastError());
			for (int64_t r0 = 0, r1 = std::min<int64_t>(ntotal, PQ_ROWS_PER_WG); r0 < ntotal; r0 = r1, r1 = std::min(ntotal, 3 * r1))
				scan_range(c, r0, r1, r1 == ntotal);
			const int64_t tot = c.nqc * k;
			hipLaunchKernelGGL(pqfs_emit_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, c.list, c.len, c.k, (long long)c.nqc,
			                   metric == METRIC_IP ? 1 : 0, c.qa, c.qb, raw_labels ? nullptr : (const long long *)d_idmap, (long long)label_offset, d_D + q0 * k,
			                   (long long *)(d_I + q0 * k));
			MVS_HIP(hipGetLastError());
		}
	}
	void search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, hipStream_t st) override {
		search_mapped(nq, d_x, k, d_D, d_I, params, nullptr, st);
	}
	bool named_stat(const char *name, int64_t *value) override {
		if (!strcmp(name, "pqfs_query_block"))
			*value = 16 * query_tiles();
		else if (!strcmp(name, "pqfs_scan_launches"))
			*value = last_ranges;
		else if (!strcmp(name, "pqfs_scan_rescans"))
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
			throw_faiss("mvs::PQFSIndex::get_centroids", __FILE__, "the index is not trained");
		MVS_HIP(hipStreamSynchronize(stream));
		MVS_HIP(hipMemcpy(out, d_cb(), cb_floats() * sizeof(float), hipMemcpyDeviceToHost));
	}
	void get_codes(int64_t row0, int64_t n, uint8_t *out) { // FAISS's packing, [n][M / 2]
		use_device();
		if (row0 < 0 || n < 0 || row0 + n > ntotal)
			throw_faiss("mvs::PQFSIndex::get_codes", __FILE__, "rows [%lld, %lld) are outside the index (ntotal %lld)", (long long)row0,
			            (long long)(row0 + n), (long long)ntotal);
		if (n == 0)
			return;
		const size_t bytes = (size_t)n * (M / 2);
		ws_pack.reserve(bytes);
		hipLaunchKernelGGL(pqfs_unpack_kernel, dim3((unsigned)((bytes + 255) / 256)), dim3(256), 0, stream, (const unsigned *)d_codes(), chunks, (long long)row0,
		                   (long long)n, M, (unsigned char *)ws_pack.p);
		MVS_HIP(hipGetLastError());
		MVS_HIP(hipStreamSynchronize(stream));
		MVS_HIP(hipMemcpy(out, ws_pack.p, bytes, hipMemcpyDeviceToHost));
	}
	// the image is this path's own (clone, to_gpu): write_index refuses the kind (csrc/index_io.hip)
	void to_host(HostIndex &out) override {
		out.kind = MVS_KIND_PQFS;
		out.d = d;
		out.metric = metric;
		out.metric_arg = metric_arg;
		out.ntotal = ntotal;
		out.is_trained = is_trained;
		out.pq_M = M;
		out.pq_centroids.assign(cb_floats(), 0.f);
		if (is_trained)
			get_centroids(out.pq_centroids.data());
		out.pq_codes.resize((size_t)ntotal * (M / 2));
		get_codes(0, ntotal, out.pq_codes.data());
	}
	void load_image(const HostIndex &h) {
		if (h.pq_centroids.size() != cb_floats() || (int64_t)h.pq_codes.size() != h.ntotal * (M / 2))
			throw_faiss("mvs::PQFSIndex::load_image", __FILE__, "PQ<M>x4fs image: %zu centroid values and %zu code bytes do not match d = %d, M = %d, "
			            "ntotal = %lld", h.pq_centroids.size(), h.pq_codes.size(), d, M, (long long)h.ntotal);
		use_device();
		metric_arg = h.metric_arg;
		if (h.is_trained)
			set_centroids(h.pq_centroids.data());
		if (h.ntotal > 0) {
			check_add(h.ntotal);
			grow(h.ntotal);
			ws_pack.reserve(h.pq_codes.size());
			MVS_HIP(hipMemcpyAsync(ws_pack.p, h.pq_codes.data(), h.pq_codes.size(), hipMemcpyHostToDevice, stream));
			hipLaunchKernelGGL(pqfs_pack_kernel, dim3(lane_grid(h.ntotal)), dim3(256), 0, stream, (const unsigned char *)ws_pack.p, (long long)h.ntotal, M, d_codes(),
			                   chunks, 0ll);
			MVS_HIP(hipGetLastError());
			MVS_HIP(hipStreamSynchronize(stream));
		}
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
		cb_.release();
		h_flag.release();
		store.release();
		release_all();
		selector.release();
		move_stream(new_device);
		ntotal = 0;
		load_image(img);
	}
	IndexBase *clone(int on_device) override {
		HostIndex img;
		to_host(img);
		IndexBase *c = pqfs_from_host(img, on_device);
		c->label_offset = label_offset;
		return c;
	}
};

PQFSIndex *as_pqfs(IndexBase *ix) {
	return ix->kind == MVS_KIND_PQFS ? static_cast<PQFSIndex *>(ix) : nullptr;
}

} // namespace

// "PQ<M>x4fs" (faiss/index_factory.cpp), called by make_pq_index with the string's M
IndexBase *make_pqfs_index(int d, long M, const std::string &desc, int metric) {
	const char *fn = "faiss::Index* faiss::index_factory(int, const char*, faiss::MetricType)";
	if (M % 2 != 0) // (FAISS packs two codes a byte: IndexFastScan asserts an even M)
		throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s (an even number of subquantizers only)",
		            desc.c_str());
	if (M > PQFS_MAX_M)
		throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s (at most %d subquantizers)",
		            desc.c_str(), PQFS_MAX_M);
	if (d % M != 0)
		throw_faiss("faiss::ProductQuantizer::set_derived_values()", "faiss/impl/ProductQuantizer.cpp",
		            "Error: 'd %% M == 0' failed: The dimension of the vector (d) should be a multiple of the number of subquantizers (M)");
	return new PQFSIndex(d, (int)M, metric);
}
IndexBase *pqfs_from_host(const HostIndex &h, int device) {
	CtorDevice scope(device);
	if (h.pq_M <= 0 || h.pq_M % 2 != 0 || h.pq_M > PQFS_MAX_M || h.d % h.pq_M != 0)
		throw_faiss("mvs::pqfs_from_host", __FILE__, "PQ<M>x4fs image with M = %d at d = %d is not served on the MI355X path", h.pq_M, h.d);
	auto *p = new PQFSIndex(h.d, h.pq_M, h.metric);
	try {
		p->load_image(h);
	} catch (...) {
		delete p;
		throw;
	}
	return p;
}
bool pqfs_info(const IndexBase *ix, int *M, int *nbits) {
	if (ix->kind != MVS_KIND_PQFS)
		return false;
	if (M)
		*M = static_cast<const PQFSIndex *>(ix)->M;
	if (nbits)
		*nbits = 4;
	return true;
}
bool pqfs_get_centroids(IndexBase *ix, float *out) {
	PQFSIndex *p = as_pqfs(ix);
	if (p)
		p->get_centroids(out);
	return p != nullptr;
}
bool pqfs_set_centroids(IndexBase *ix, const float *c) {
	PQFSIndex *p = as_pqfs(ix);
	if (p)
		p->set_centroids(c);
	return p != nullptr;
}
bool pqfs_get_codes(IndexBase *ix, int64_t row0, int64_t n, uint8_t *out) {
	PQFSIndex *p = as_pqfs(ix);
	if (p)
		p->get_codes(row0, n, out);
	return p != nullptr;
}

} // namespace mvs
