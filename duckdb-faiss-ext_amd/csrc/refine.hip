// csrc/refine.hip -- "<base>,RFlat" / "<base>,Refine(Flat)" (faiss::IndexRefineFlat): a compressed base index proposes k * k_factor candidates,
// a Flat copy of the rows re-scores them in FAISS's f32 pair-path arithmetic and the best k are returned with exact distances.
//
// Contract (include/mi355_faiss.h "exact f32 re-ranking over the quantised indexes"):
//   base    one of PQ<M>, IVF<n>,PQ<M>, SQ8, IVF<n>,SQ8 (csrc/pq.hip, csrc/ivfpq.hip, csrc/sq.hip), searched with IndexBase::raw_labels set: its
//           labels are row numbers of the store (an id map only feeds its selector); its label_offset stays 0 and it never sees ids
//   store   a FlatIndex with the same rows in arrival order: ingest staging, growth and file images are FlatIndex's; it is never searched,
//           so none of its coarse stores is ever built
//   search  kb = (int64)((float)k * k_factor) <= 2048 candidates per query from the base, then refine_flat_kernel
//
// refine_flat_kernel<NL, L2, IL>: one workgroup of 256 lanes per query.
//   1. the query goes to LDS (zero padded to a multiple of four components)
//   2. the candidates are taken in tiles of TR = 16 NL rows (64 | 128 | 256, the smallest that holds kb, else 256) and the rows in chunks of
//      at most 64 components: 16 consecutive lanes read one row's 256 bytes of the chunk, 16 bytes a lane; a lane issues all its NL loads
//      (4 NL rows in flight per wave, <= 64 KB per workgroup) before the first is written to the LDS tile.  Row pitch 68 floats: lane i's
//      16-byte reads at 68 i floats fall into 16 distinct bank quads per group of 16 lanes (as the 132 of ivf_bucket_exact_kernel)
//   3. lane i walks candidate i's chain over the chunk from LDS, the query by broadcast reads; acc is carried across the chunks.  The
//      pair-interleaved store (FlatGeom) is un-swapped by bit 4 of the ROW NUMBER
//   4. key = (order bits of the exact value << 32) | row into the key array in LDS; after the last tile a bitonic sort of P = 2^ceil(log2 kb)
//      keys; a -1 candidate's key is all ones and sorts behind every real one
//   5. the first k keys are written as distances and labels (label_offset + row, or id_map[row])
// No second launch, no k-lists in global memory, no scratch.
#include "pq_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace mvs {

namespace {

constexpr int RF_THREADS = 256;
constexpr int RF_KC = 64;                                // components per staged chunk
constexpr int RF_PITCH = RF_KC + 4;                      // LDS row pitch in floats
constexpr int RF_MAX_KB = PQ_MAX_K;                      // the bases serve k <= 2048
constexpr size_t RF_CAND_SCRATCH = (size_t)256 << 20;    // the base's candidate lists of one pass
constexpr size_t RF_CAND_BYTES = sizeof(float) + sizeof(int64_t);

struct RefineArgs {
	const float *x;        // [nq][d]
	const long long *cand; // [nq][kb] store rows, -1 padded
	const float *rows;     // the store: [nrows][dp]
	long long nrows;
	int d, dp, kb, k, P;
	const long long *idmap;
	long long label_offset;
	float *D;     // [nq][k]
	long long *I; // [nq][k]
};

inline int refine_tile_loads(int64_t kb) {
	return kb <= 64 ? 4 : (kb <= 128 ? 8 : 16);
}
inline size_t refine_lds_bytes(int NL, int d, int P) {
	return (size_t)16 * NL * RF_PITCH * sizeof(float) + (size_t)((d + 3) / 4 * 4) * sizeof(float) + (size_t)P * sizeof(unsigned long long) +
	       (size_t)16 * NL * sizeof(int);
}

// four components of the chain; n < 4: only the first n (the row's last, partial group)
template <bool L2>
__device__ __forceinline__ float refine_step4(float acc, const float4 xv, const float4 yv, bool il, bool flip, int n) {
	const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
	float ys[4] = {yv.x, yv.y, yv.z, yv.w};
	if (il) { // stored [k0,k2,k1,k3] (bit 4 of the row clear) or [k1,k3,k0,k2]
		ys[0] = flip ? yv.z : yv.x, ys[1] = flip ? yv.x : yv.z, ys[2] = flip ? yv.w : yv.y, ys[3] = flip ? yv.y : yv.w;
	}
#pragma unroll
	for (int e = 0; e < 4; ++e) {
		if (e < n) {
			if (L2) {
				const float t = __fsub_rn(xs[e], ys[e]);
				acc = fmaf(t, t, acc);
			} else {
				acc = fmaf(xs[e], ys[e], acc);
			}
		}
	}
	return acc;
}

template <int NL, bool L2, bool IL>
__global__ __launch_bounds__(RF_THREADS) void refine_flat_kernel(const RefineArgs a) {
	constexpr int TR = 16 * NL; // candidates per tile
	extern __shared__ __attribute__((aligned(16))) float rf_lds[];
	float *tile = rf_lds;                                                             // [TR][RF_PITCH]
	float *xq = tile + TR * RF_PITCH;                                                 // [ceil4(d)]
	unsigned long long *keys = reinterpret_cast<unsigned long long *>(xq + (a.d + 3) / 4 * 4); // [P]
	int *s_row = reinterpret_cast<int *>(keys + a.P);                                 // [TR]
	const int tid = threadIdx.x, d = a.d, dp = a.dp, kb = a.kb;
	const long long q = blockIdx.x;
	for (int j = tid; j < (d + 3) / 4 * 4; j += RF_THREADS)
		xq[j] = j < d ? a.x[q * d + j] : 0.f;
	for (int i = tid; i < a.P; i += RF_THREADS)
		keys[i] = ~0ull;
	const long long *cq = a.cand + q * kb;
	for (int t0 = 0; t0 < kb; t0 += TR) { // (uniform trip counts throughout: every lane reaches every barrier)
		__syncthreads();                  // (the previous tile's rows and row numbers have been read; first trip: xq and keys are written)
		if (tid < TR) {
			long long r = t0 + tid < kb ? cq[t0 + tid] : -1;
			if (r < 0 || r >= a.nrows) // (a candidate outside the store is no candidate: nothing is read through it)
				r = -1;
			s_row[tid] = (int)r;
		}
		__syncthreads();
		const int myrow = tid < TR ? s_row[tid] : -1;
		const bool flip = IL && ((myrow >> 4) & 1);
		float acc = 0.f;
		for (int c0 = 0; c0 < d; c0 += RF_KC) {
			const int cw = dp - c0 < RF_KC ? dp - c0 : RF_KC;      // stored floats of the chunk: 8 | 16 | 32 | 64
			const int pr = cw >> 2, prs = 31 - __clz(pr);          // 16-byte pieces per row, a power of two
			if (c0 > 0)
				__syncthreads(); // (the previous chunk's tile has been read)
			float4 v[NL];
			int at[NL];
#pragma unroll
			for (int it = 0; it < NL; ++it) { // every load is issued before the first is consumed
				const int f = it * RF_THREADS + tid, r = f >> prs, pc = f & (pr - 1);
				const int row = r < TR ? s_row[r] : -1;
				at[it] = row >= 0 ? r * RF_PITCH + pc * 4 : -1;
				v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
				if (row >= 0)
					v[it] = *reinterpret_cast<const float4 *>(a.rows + (size_t)row * dp + c0 + pc * 4);
			}
#pragma unroll
			for (int it = 0; it < NL; ++it)
				if (at[it] >= 0)
					*reinterpret_cast<float4 *>(tile + at[it]) = v[it];
			__syncthreads();
			if (myrow >= 0) {
				const int nc = d - c0 < cw ? d - c0 : cw; // logical components of the chunk
				const float *y = tile + tid * RF_PITCH, *xc = xq + c0;
				int g = 0;
#pragma unroll 4
				for (; g + 4 <= nc; g += 4)
					acc = refine_step4<L2>(acc, *reinterpret_cast<const float4 *>(xc + g), *reinterpret_cast<const float4 *>(y + g), IL, flip, 4);
				if (g < nc)
					acc = refine_step4<L2>(acc, *reinterpret_cast<const float4 *>(xc + g), *reinterpret_cast<const float4 *>(y + g), IL, flip, nc - g);
			}
		}
		if (myrow >= 0)
			keys[t0 + tid] = ((unsigned long long)pq_key(acc, L2 ? 0 : 1) << 32) | (unsigned long long)(unsigned)myrow;
	}
	__syncthreads();
	for (int kk = 2; kk <= a.P; kk <<= 1)
		for (int j = kk >> 1; j > 0; j >>= 1) {
			for (int i = tid; i < a.P; i += RF_THREADS) {
				const int p = i ^ j;
				if (p > i) {
					const unsigned long long ka = keys[i], kc = keys[p];
					if ((ka > kc) == ((i & kk) == 0)) {
						keys[i] = kc;
						keys[p] = ka;
					}
				}
			}
			__syncthreads();
		}
	for (int s = tid; s < a.k; s += RF_THREADS) {
		const unsigned long long e = s < a.P ? keys[s] : ~0ull;
		float dv = L2 ? FLT_MAX : -FLT_MAX;
		long long lab = -1;
		if (e != ~0ull) {
			const long long row = (long long)(e & 0xFFFFFFFFull);
			dv = pq_unkey((unsigned)(e >> 32), L2 ? 0 : 1);
			lab = a.idmap ? a.idmap[row] : row + a.label_offset;
		}
		a.D[q * a.k + s] = dv;
		a.I[q * a.k + s] = lab;
	}
}

bool refine_base_kind(int kind) {
	return kind == MVS_KIND_PQ || kind == MVS_KIND_IVFPQ || kind == MVS_KIND_SQ || kind == MVS_KIND_IVFSQ;
}
void check_device_id(int dev) {
	int ndev = 0;
	MVS_HIP(hipGetDeviceCount(&ndev));
	if (dev < 0 || dev >= ndev)
		throw_faiss("faiss::gpu::index_cpu_to_gpu", "faiss/gpu/GpuCloner.cpp", "Invalid GPU device %d", dev);
}

// ---------------------------------------------------------------------------------------------- index
class RefineIndex : public IndexBase {
public:
	IndexBase *base;  // owned
	FlatIndex *store; // owned
	float k_factor = 1.f;
	DevBuf ws_cD, ws_cI;
	int64_t last_kb = 0, last_chunk = 0;

	RefineIndex(IndexBase *base_, FlatIndex *store_) : IndexBase(MVS_KIND_REFINE, base_->d, base_->metric), base(base_), store(store_) {
		base->raw_labels = true;
		is_trained = base->is_trained;
		ntotal = store->ntotal;
	}
	~RefineIndex() override {
		(void)hipSetDevice(device);
		if (stream)
			(void)hipStreamSynchronize(stream);
		delete base;
		delete store;
	}
	void adopt_tuning(const Tuning &t) override {
		tune_ = t;
		base->adopt_tuning(t);
		store->adopt_tuning(t);
	}
	void refresh_trained() override {
		base->refresh_trained();
		is_trained = base->is_trained;
	}
	void train(int64_t n, const float *x) override {
		base->train(n, x);
		is_trained = base->is_trained;
	}
	// the base first (it fails on an untrained index with its own 'is_trained' message, before a row moves): a throw leaves the store unchanged
	void add(int64_t n, const float *x) override {
		if (n <= 0)
			return;
		base->add(n, x);
		store->add(n, x);
		ntotal = store->ntotal;
		is_trained = base->is_trained;
	}
	void add_device(int64_t n, const float *d_x, hipStream_t st) override {
		if (n <= 0)
			return;
		base->add_device(n, d_x, st);
		store->add_device(n, d_x, st);
		ntotal = store->ntotal;
		is_trained = base->is_trained;
	}
	// (add_with_ids / add_with_ids_device: IndexBase's "add_with_ids not implemented for this type of index")

	static int64_t candidates(int64_t k, float k_factor) {
		return (int64_t)((float)k * k_factor); // an f32 product, truncated
	}
	void search_mapped(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, const int64_t *d_idmap,
	                   hipStream_t st) override {
		use_device();
		refresh_trained();
		if (k <= 0)
			throw_faiss("virtual void faiss::IndexRefine::search(...) const", "faiss/IndexRefine.cpp", "Error: 'k > 0' failed");
		const int64_t kb = candidates(k, k_factor);
		if (kb > RF_MAX_KB)
			throw_faiss("mvs::RefineIndex::search", __FILE__, "k = %lld with k_factor = %g asks the base index for %lld candidates: beyond the %d a "
			            "refine stage serves on the MI355X path", (long long)k, (double)k_factor, (long long)kb, RF_MAX_KB);
		if (nq <= 0)
			return;
		const int64_t nq_chunk = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(RF_CAND_SCRATCH / ((size_t)kb * RF_CAND_BYTES))));
		last_kb = kb, last_chunk = nq_chunk;
		ws_cD.reserve((size_t)nq_chunk * kb * sizeof(float));
		ws_cI.reserve((size_t)nq_chunk * kb * sizeof(int64_t));
		store->use_device();
		store->flush_adds();           // staged rows reach the device (on the store's stream)
		store->reap_retired(false);
		stream_wait(st, store->stream);
		const FlatGeom &g = store->geom;
		const int NL = refine_tile_loads(kb);
		int P = 1;
		while (P < kb)
			P <<= 1;
		const size_t lds = refine_lds_bytes(NL, d, P);
		RefineArgs a;
		a.cand = (const long long *)ws_cI.p;
		a.rows = store->vecs();
		a.nrows = store->ntotal;
		a.d = d, a.dp = g.dp, a.kb = (int)kb, a.k = (int)k, a.P = P;
		a.idmap = (const long long *)d_idmap;
		a.label_offset = label_offset;
		const bool l2 = metric == METRIC_L2, il = g.pair_interleaved;
		memset(&kinfo, 0, sizeof kinfo);
		for (int64_t q0 = 0; q0 < nq; q0 += nq_chunk) {
			const int64_t nqc = std::min(nq_chunk, nq - q0);
			base->search_mapped(nqc, d_x + q0 * d, kb, (float *)ws_cD.p, (int64_t *)ws_cI.p, params, d_idmap, st);
			use_device();
			a.x = d_x + q0 * d;
			a.D = d_D + q0 * k;
			a.I = (long long *)(d_I + q0 * k);
			const dim3 grid((unsigned)nqc);
			begin_kernel_timing(st);
#define RF_LAUNCH(NN, LL, II)                                                                                                                       \
	do {                                                                                                                                            \
		ensure_dynamic_lds((const void *)refine_flat_kernel<NN, LL, II>, lds);                                                                      \
		hipLaunchKernelGGL((refine_flat_kernel<NN, LL, II>), grid, dim3(RF_THREADS), lds, st, a);                                                   \
	} while (0)
#define RF_LAUNCH_N(LL, II)                                                                                                                         \
	do {                                                                                                                                            \
		if (NL == 4)                                                                                                                                \
			RF_LAUNCH(4, LL, II);                                                                                                                   \
		else if (NL == 8)                                                                                                                           \
			RF_LAUNCH(8, LL, II);                                                                                                                   \
		else                                                                                                                                        \
			RF_LAUNCH(16, LL, II);                                                                                                                  \
	} while (0)
			if (l2 && il)
				RF_LAUNCH_N(true, true);
			else if (l2)
				RF_LAUNCH_N(true, false);
			else if (il)
				RF_LAUNCH_N(false, true);
			else
				RF_LAUNCH_N(false, false);
#undef RF_LAUNCH_N
#undef RF_LAUNCH
			MVS_HIP(hipGetLastError());
			end_kernel_timing(st);
			// the stage's roofline: every candidate row fetched once, whole (an upper bound where lists are short of kb)
			const double kbv = (double)std::min<int64_t>(kb, store->ntotal);
			set_kinfo("refine_flat_kernel", (double)nqc * kbv * d * (l2 ? 3.0 : 2.0), (double)nqc * kbv * 4.0 * g.dp, (int)nqc, RF_THREADS, (int)lds, 1);
			if (q0 + nq_chunk < nq)
				MVS_HIP(hipStreamSynchronize(st)); // (the next pass overwrites the candidate lists)
		}
	}
	void search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, hipStream_t st) override {
		search_mapped(nq, d_x, k, d_D, d_I, params, nullptr, st);
	}
	// faiss::IndexRefine::reconstruct: the refine store's f32 row
	void recon_source(ReconSource &src, hipStream_t st) override {
		store->recon_source(src, st);
		use_device();
	}
	bool set_option(const char *key, int64_t v) override {
		return base->set_option(key, v);
	}
	bool named_stat(const char *name, int64_t *value) override {
		if (!strcmp(name, "refine_candidates"))
			*value = last_kb;
		else if (!strcmp(name, "refine_store_bytes"))
			*value = (int64_t)device_bytes();
		else if (!strcmp(name, "refine_query_chunk"))
			*value = last_chunk;
		else
			return base->named_stat(name, value);
		return true;
	}
	size_t device_bytes() const override { // the store's f32 rows
		return (size_t)store->cap * store->geom.dp * sizeof(float);
	}

	// ------------------------------------------------------------------------------------------ images, placement
	void to_host(HostIndex &out) override {
		refresh_trained();
		out.kind = MVS_KIND_REFINE;
		out.d = d;
		out.metric = metric;
		out.metric_arg = metric_arg;
		out.ntotal = ntotal;
		out.is_trained = is_trained;
		out.sub.reset(new HostIndex);
		base->to_host(*out.sub);
		out.sub2.reset(new HostIndex);
		store->to_host(*out.sub2);
		out.k_factor = k_factor;
	}
	void to_device(int new_device) override {
		if (new_device == device)
			return;
		check_device_id(new_device);
		base->to_device(new_device);
		store->to_device(new_device);
		use_device();
		MVS_HIP(hipStreamSynchronize(stream));
		ws_cD.release();
		ws_cI.release();
		move_stream(new_device);
	}
	IndexBase *clone(int on_device) override {
		check_device_id(on_device);
		HostIndex img;
		to_host(img);
		IndexBase *c = refine_from_host(img, on_device);
		c->label_offset = label_offset;
		return c;
	}
};

RefineIndex *as_refine(IndexBase *ix) {
	return ix && ix->kind == MVS_KIND_REFINE ? static_cast<RefineIndex *>(ix) : nullptr;
}

} // namespace

// "<base>,RFlat" | "<base>,Refine(Flat)" (faiss/index_factory.cpp: the refine suffix is the string's last component); nullptr if desc has no
// refine suffix.  `full` is the whole factory string, for the messages
IndexBase *make_refine_index(int d, const std::string &desc, int metric, const std::string &full) {
	const char *fn = "faiss::Index* faiss::index_factory(int, const char*, faiss::MetricType)";
	const size_t comma = desc.rfind(',');
	if (comma == std::string::npos)
		return nullptr;
	const std::string tail = desc.substr(comma + 1), head = desc.substr(0, comma);
	if (tail != "RFlat" && tail.rfind("Refine(", 0) != 0)
		return nullptr;
	if (tail != "RFlat" && tail != "Refine(Flat)") // Refine(SQ8), Refine(PQ16), ...: only the Flat store
		throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s (Flat refine store only)", full.c_str());
	if (metric != METRIC_L2 && metric != METRIC_IP)
		throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s with metric type %d (L2 and inner "
		            "product only)", full.c_str(), metric);
	// the base: one of the four scanning kinds, by its own maker (which refuses what it does not serve in its own words)
	IndexBase *base = nullptr;
	const bool coded = head.rfind("PQ", 0) == 0 || head.rfind("SQ", 0) == 0 ||
	                   (head.rfind("IVF", 0) == 0 && (head.find(",PQ") != std::string::npos || head.find(",SQ") != std::string::npos));
	if (coded && head.find("RFlat") == std::string::npos && head.find("Refine(") == std::string::npos) {
		base = make_ivfpq_index(d, head, metric);
		if (!base)
			base = make_sq_index(d, head, metric);
		if (!base)
			base = make_pq_index(d, head, metric);
	}
	if (!base || !refine_base_kind(base->kind)) { // Flat, IVF<n>,Flat, HNSW..., a second refine stage, ...
		delete base;
		throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s (a refine stage over PQ<M>, "
		            "IVF<n>,PQ<M>, SQ8 or IVF<n>,SQ8 only)", full.c_str());
	}
	FlatIndex *store = nullptr;
	try {
		store = new FlatIndex(d, metric);
		return new RefineIndex(base, store);
	} catch (...) {
		delete store;
		delete base;
		throw;
	}
}

IndexBase *refine_from_host(const HostIndex &h, int device) {
	const char *fn = "faiss::Index* faiss::read_index(...)", *file = "faiss/impl/index_read.cpp";
	if (!h.sub || !h.sub2)
		throw_faiss(fn, file, "IndexRefine image without its two sub-indexes");
	const HostIndex &b = *h.sub, &s = *h.sub2;
	if (s.kind != MVS_KIND_FLAT)
		throw_faiss(fn, file, "IndexRefine whose refine index is not a Flat image (\"IxF2\" / \"IxFI\") is not implemented on the MI355X path");
	if (!refine_base_kind(b.kind))
		throw_faiss(fn, file, "IndexRefine over a base index of kind %d is not implemented on the MI355X path (PQ, IVFPQ, SQ8 and IVFSQ8 only)", b.kind);
	if (b.d != s.d || b.metric != s.metric || b.ntotal != s.ntotal)
		throw_faiss(fn, file, "IndexRefine image: base index (d = %d, metric %d, ntotal = %lld) and refine index (d = %d, metric %d, ntotal = %lld) "
		            "disagree", b.d, b.metric, (long long)b.ntotal, s.d, s.metric, (long long)s.ntotal);
	if (b.metric != METRIC_L2 && b.metric != METRIC_IP)
		throw_faiss(fn, file, "IndexRefine with metric type %d is not implemented on the MI355X path", b.metric);
	for (const auto &l : b.list_ids) // IVF bases: a stored id is a row number of the store
		for (int64_t id : l)
			if (id < 0 || id >= s.ntotal)
				throw_faiss(fn, file, "IndexRefine image: the base index holds the stored id %lld outside [0, %lld): its ids must be row numbers of "
				            "the refine index", (long long)id, (long long)s.ntotal);
	if (!(h.k_factor >= 1.f))
		throw_faiss(fn, file, "IndexRefine image with k_factor = %g", (double)h.k_factor);
	CtorDevice scope(device);
	IndexBase *base = index_from_host(b, device);
	IndexBase *store = nullptr;
	RefineIndex *r = nullptr;
	try {
		store = index_from_host(s, device);
		r = new RefineIndex(base, static_cast<FlatIndex *>(store));
	} catch (...) {
		delete store;
		delete base;
		throw;
	}
	r->k_factor = h.k_factor;
	r->metric_arg = h.metric_arg;
	return r;
}
IndexBase *refine_base_of(IndexBase *ix) {
	RefineIndex *p = as_refine(ix);
	return p ? p->base : nullptr;
}
IndexBase *refine_store_of(IndexBase *ix) {
	RefineIndex *p = as_refine(ix);
	return p ? p->store : nullptr;
}
bool refine_set_k_factor(IndexBase *ix, float k_factor) {
	RefineIndex *p = as_refine(ix);
	if (!p)
		return false;
	if (!(k_factor >= 1.f) || std::isinf(k_factor))
		throw_faiss("mvs_index_refine_set_k_factor", __FILE__, "k_factor = %g: the refine stage needs k_factor >= 1", (double)k_factor);
	p->k_factor = k_factor;
	return true;
}
bool refine_get_k_factor(IndexBase *ix, float *k_factor) {
	RefineIndex *p = as_refine(ix);
	if (p && k_factor)
		*k_factor = p->k_factor;
	return p != nullptr;
}

} // namespace mvs
