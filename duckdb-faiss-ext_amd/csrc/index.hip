// csrc/index.hip -- device-native index objects + the C ABI of include/mi355_faiss.h.
//
// Host side of the hot path.  Mirrors the FAISS object graph the reference's glue walks
// (/root/reference/src/faiss_extension.cpp:123-144 setIndexParameters, :668-721 innerCreateSearchParameters):
//   FlatIndex     <- faiss::IndexFlat{L2,IP}      rows in HBM, padded row-major + per-row squared norms
//   IDMapIndex    <- faiss::IndexIDMap            int64 id_map in HBM, translated in the merge kernel
//   IVFFlatIndex  <- faiss::IndexIVFFlat          (csrc/ivf.hip)
// Every index owns a HIP stream and a ring of pinned staging buffers: add() copies the caller's rows into
// pinned memory (the caller's DataChunk buffer is only valid during the call, :493-512) and returns while
// hipMemcpyAsync + the norm kernel run on the stream.
#include "coded_lists.h"
#include "flat_collect.h"
#include "collect_launch.h"
#include "index.h"

#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <optional>
#include <thread>

#include <algorithm>
#include <dlfcn.h>
#include <chrono>
#include <cstdarg>
#include <cstdlib>
#include <cstring>

namespace mvs {

static thread_local std::string g_last_error;

void set_last_error(const char *what) { // (csrc/binary.hip's entry points report through the same mvs_last_error)
	g_last_error = what;
}

void throw_faiss(const char *func, const char *file, const char *fmt, ...) {
	char msg[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(msg, sizeof msg, fmt, ap);
	va_end(ap);
	// FAISS: "Error in <func> at <file>:<line>: <msg>" (impl/FaissException.cpp)
	const char *base = strrchr(file, '/');
	throw Error(std::string("Error in ") + func + " at " + (base ? base + 1 : file) + ": " + msg);
}

// ------------------------------------------------------------------------------------------ buffers

PinnedRing::~PinnedRing() {
	for (int i = 0; i < NB; ++i) {
		if (buf[i])
			(void)hipHostFree(buf[i]);
		if (ev[i])
			(void)hipEventDestroy(ev[i]);
	}
}
void PinnedRing::drop_events() { // (the owner moves to another device: events are created again, there, by the next acquire)
	for (int i = 0; i < NB; ++i)
		if (ev[i]) {
			(void)hipEventSynchronize(ev[i]);
			(void)hipEventDestroy(ev[i]);
			ev[i] = nullptr;
		}
}
// The staging copy of add(): pageable rows -> a pinned slot that only the copy engine reads afterwards.  Non-temporal stores skip
// the read-for-ownership of the destination lines (tools/micro/h2d_chunks.cpp on the GPU box, 1 MB chunks: 23.9 us against memcpy's
// 35.5; with the hipMemcpyAsync behind it 30.0 against 26.4 GB/s).  dst is 16-byte aligned (slots are page aligned), src need not be.
static void stage_copy(void *dst, const void *src, size_t bytes) {
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
	if ((uintptr_t)dst & 15) { // (chunks of rows whose size is no multiple of 16 bytes follow each other unaligned: plain copy)
		memcpy(dst, src, bytes);
		return;
	}
	typedef float v4f __attribute__((ext_vector_type(4)));
	const size_t n16 = bytes / 16;
	const char *s = (const char *)src;
	v4f *d = (v4f *)dst;
	for (size_t i = 0; i < n16; ++i) {
		v4f v;
		memcpy(&v, s + 16 * i, 16);
		__builtin_nontemporal_store(v, d + i);
	}
	if (bytes & 15)
		memcpy((char *)dst + 16 * n16, s + 16 * n16, bytes & 15);
	__builtin_ia32_sfence(); // (the stores are weakly ordered: visible before the copy engine is told to read)
#else
	memcpy(dst, src, bytes);
#endif
}
// Round 6: a chunk of the glue's size (1 MB) is copied by THREE threads (MVS_STAGE_THREADS).  The call runs under the glue's faiss_lock and seven of eight
// calls are nothing but this copy (profiles/r6_ingest.txt: 36 us per MB with the other workers filling their next chunks, the
// ceiling of the call pattern); helper threads that take the other parts shorten exactly that.  A helper spins between the
// calls of an ingest burst (they follow each other within ~50 us) and goes to sleep 300 us after the last one; callers of different
// indexes do not queue for the helpers (try_lock: the loser copies alone).  MVS_STAGE_THREADS=1 keeps the copy on the calling thread.
namespace {
struct StageHelper {
	std::atomic<uint64_t> seq {0}, done {0};
	const void *src = nullptr;
	void *dst = nullptr;
	size_t bytes = 0;
	std::atomic<bool> sleeping {false};
	std::mutex mu;
	std::condition_variable cv;
	void run() {
		uint64_t seen = 0;
		for (;;) {
			const auto t0 = std::chrono::steady_clock::now();
			unsigned spins = 0;
			while (seq.load(std::memory_order_acquire) == seen) {
				__builtin_ia32_pause();
				if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(300)) {
					std::unique_lock<std::mutex> lk(mu);
					sleeping.store(true, std::memory_order_release);
					cv.wait(lk, [&] { return seq.load(std::memory_order_acquire) != seen; });
					sleeping.store(false, std::memory_order_release);
				}
			}
			seen = seq.load(std::memory_order_acquire);
			stage_copy(dst, src, bytes);
			done.store(seen, std::memory_order_release);
		}
	}
	void wake() {
		if (sleeping.load(std::memory_order_acquire)) {
			{ std::lock_guard<std::mutex> lk(mu); }
			cv.notify_one();
		}
	}
};
} // namespace
// dst <- src with the helpers' hands where it pays (>= 256 KB, 16-byte aligned parts); MVS_STAGE_THREADS = copying threads in all (1 .. 4)
static void stage_copy_mt(void *dst, const void *src, size_t bytes) {
	static const int nthreads = []() {
		const char *e = getenv("MVS_STAGE_THREADS");
		const int v = e ? atoi(e) : 3;
		return v < 1 ? 1 : (v > 4 ? 4 : v);
	}();
	static std::mutex owner; // (callers of different indexes do not queue for the helpers: the loser copies alone)
	static StageHelper *helpers[3] = {nullptr, nullptr, nullptr};
	if (nthreads <= 1 || bytes < ((size_t)256 << 10) || ((uintptr_t)dst & 15) || !owner.try_lock()) {
		stage_copy(dst, src, bytes);
		return;
	}
	const int nh = nthreads - 1;
	const size_t part = (bytes / (size_t)nthreads) & ~(size_t)63;
	uint64_t job[3];
	for (int i = 0; i < nh; ++i) {
		if (!helpers[i]) {
			helpers[i] = new StageHelper; // (never destroyed: its thread may outlive static destruction)
			StageHelper *hp = helpers[i];
			std::thread([hp]() { hp->run(); }).detach();
		}
		StageHelper &h = *helpers[i];
		const size_t off = part * (size_t)(i + 1), len = i + 1 == nh ? bytes - off : part;
		h.src = (const char *)src + off, h.dst = (char *)dst + off, h.bytes = len;
		job[i] = h.seq.fetch_add(1, std::memory_order_acq_rel) + 1;
		h.wake();
	}
	stage_copy(dst, src, part);
	for (int i = 0; i < nh; ++i) {
		StageHelper &h = *helpers[i];
		unsigned spins = 0;
		while (h.done.load(std::memory_order_acquire) != job[i]) {
			__builtin_ia32_pause();
			if ((++spins & 4095u) == 0)
				h.wake(); // (the helper was on its way to sleep when the job was posted)
		}
	}
	owner.unlock();
}
int PinnedRing::acquire(size_t bytes) {
	const int i = next;
	next = (next + 1) % NB;
	if (!ev[i])
		MVS_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
	else
		MVS_HIP(hipEventSynchronize(ev[i])); // previous copy out of this slot has finished
	if (bytes > cap[i]) {
		if (buf[i])
			MVS_HIP(hipHostFree(buf[i]));
		buf[i] = nullptr;
		size_t want = std::max(bytes, (size_t)SLOT_BYTES);
		MVS_HIP(hipHostMalloc(&buf[i], want, hipHostMallocDefault));
		cap[i] = want;
	}
	return i;
}
void PinnedRing::release(int i, hipStream_t st) {
	MVS_HIP(hipEventRecord(ev[i], st));
}

void ensure_dynamic_lds(const void *kernel, size_t bytes) {
	static std::mutex mu;
	static std::map<std::pair<int, const void *>, size_t> raised;
	int dev = 0;
	MVS_HIP(hipGetDevice(&dev));
	std::lock_guard<std::mutex> g(mu);
	size_t &cur = raised[{dev, kernel}];
	if (bytes > cur) {
		MVS_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
		cur = bytes;
	}
}

// ------------------------------------------------------------------------------------------ base

static thread_local int tl_ctor_device = -1;
CtorDevice::CtorDevice(int dev) : prev(tl_ctor_device) {
	if (dev >= 0)
		tl_ctor_device = dev;
}
CtorDevice::~CtorDevice() {
	tl_ctor_device = prev;
}
static int env_device() {
	if (tl_ctor_device >= 0)
		return tl_ctor_device;
	const char *e = getenv("MVS_DEVICE");
	return e ? atoi(e) : 0;
}

IndexBase::IndexBase(int kind_, int d_, int metric_) : kind(kind_), d(d_), metric(metric_) {
	int ndev = 0;
	hipError_t e = hipGetDeviceCount(&ndev);
	if (e != hipSuccess || ndev <= 0)
		throw_faiss("mvs::IndexBase::IndexBase", __FILE__,
		            "no MI355X (gfx950) device is usable (%s): the MI355X vector-search path has no CPU fallback",
		            e == hipSuccess ? "device count 0" : hipGetErrorString(e));
	device = env_device();
	if (device < 0 || device >= ndev)
		throw_faiss("mvs::IndexBase::IndexBase", __FILE__, "Invalid GPU device %d", device);
	MVS_HIP(hipSetDevice(device));
	MVS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
}
IndexBase::~IndexBase() {
	forget_current_tuning(&tune_); // (the destroying thread's next launch read freed memory; other threads enter through use_device())
	if (stream) {
		(void)hipSetDevice(device);
		(void)hipStreamSynchronize(stream);
		(void)hipStreamDestroy(stream);
	}
	for (auto &p : timing_events) {
		(void)hipEventDestroy(p.first);
		(void)hipEventDestroy(p.second);
	}
}
// make stream `waiter` wait for everything enqueued so far on `signal`
void stream_wait(hipStream_t waiter, hipStream_t signal) {
	if (waiter == signal)
		return;
	hipEvent_t e;
	MVS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
	MVS_HIP(hipEventRecord(e, signal));
	MVS_HIP(hipStreamWaitEvent(waiter, e, 0));
	MVS_HIP(hipEventDestroy(e));
}

void IndexBase::use_device() const {
	MVS_HIP(hipSetDevice(device)); // DuckDB calls from arbitrary worker threads
	set_current_tuning(&tune_);    // ... and this index's tuning is what the launches of this call read (csrc/common.h Tuning)
}
void IndexBase::move_stream(int new_device) {
	pinned.drop_events();
	for (DevBuf *b : {&ws_hx, &ws_hD, &ws_hI, &ws_rkeys, &ws_rpos, &ws_rout, &ws_rmiss})
		b->release();
	MVS_HIP(hipStreamDestroy(stream));
	stream = nullptr;
	MVS_HIP(hipSetDevice(new_device));
	MVS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
	device = new_device;
}
void IndexBase::train(int64_t, const float *) {
	// faiss::Index::train: "does nothing by default"
}
void IndexBase::add_with_ids(int64_t, const float *, const int64_t *) {
	// faiss/Index.cpp -- substring matched at src/faiss_extension.cpp:523; user text pinned by faiss4.test:22
	throw_faiss("virtual void faiss::Index::add_with_ids(faiss::idx_t, const float*, const faiss::idx_t*)",
	            "faiss/Index.cpp", "add_with_ids not implemented for this type of index");
}
void IndexBase::add_with_ids_device(int64_t, const float *, const int64_t *, hipStream_t) {
	throw_faiss("virtual void faiss::Index::add_with_ids(faiss::idx_t, const float*, const faiss::idx_t*)",
	            "faiss/Index.cpp", "add_with_ids not implemented for this type of index");
}

// host-pointer search = stage queries, device search, copy back (src/faiss_extension.cpp:623-638)
void IndexBase::search(int64_t nq, const float *x, int64_t k, float *D, int64_t *I, const mvs_search_params *params) {
	use_device();
	if (k <= 0)
		throw_faiss("virtual void faiss::Index::search(...) const", "faiss/Index.cpp", "Error: 'k > 0' failed");
	if (nq <= 0)
		return;
	ws_hx.reserve((size_t)nq * d * sizeof(float));
	ws_hD.reserve((size_t)nq * k * sizeof(float));
	ws_hI.reserve((size_t)nq * k * sizeof(int64_t));
	const size_t xbytes = (size_t)nq * d * sizeof(float);
	int slot = pinned.acquire(xbytes);
	memcpy(pinned.buf[slot], x, xbytes);
	MVS_HIP(hipMemcpyAsync(ws_hx.p, pinned.buf[slot], xbytes, hipMemcpyHostToDevice, stream));
	pinned.release(slot, stream);
	search_device(nq, (const float *)ws_hx.p, k, (float *)ws_hD.p, (int64_t *)ws_hI.p, params, stream);
	const size_t dbytes = (size_t)nq * k * sizeof(float), ibytes = (size_t)nq * k * sizeof(int64_t);
	slot = pinned.acquire(dbytes + ibytes);
	char *hb = (char *)pinned.buf[slot];
	MVS_HIP(hipMemcpyAsync(hb, ws_hD.p, dbytes, hipMemcpyDeviceToHost, stream));
	MVS_HIP(hipMemcpyAsync(hb + dbytes, ws_hI.p, ibytes, hipMemcpyDeviceToHost, stream));
	MVS_HIP(hipStreamSynchronize(stream));
	memcpy(D, hb, dbytes);
	memcpy(I, hb + dbytes, ibytes);
	pinned.release(slot, stream);
}

const float *IndexBase::stage_queries(int64_t nq, const float *x) {
	const size_t xbytes = (size_t)nq * d * sizeof(float);
	ws_hx.reserve(xbytes);
	const int slot = pinned.acquire(xbytes);
	memcpy(pinned.buf[slot], x, xbytes);
	MVS_HIP(hipMemcpyAsync(ws_hx.p, pinned.buf[slot], xbytes, hipMemcpyHostToDevice, stream));
	pinned.release(slot, stream);
	return (const float *)ws_hx.p;
}
// faiss::Index::range_search (faiss/Index.cpp): the base class refuses; Flat, IVF<n>,Flat and IDMap over them override
void IndexBase::range_search(int64_t, const float *, float, const mvs_search_params *, RangeResult &) {
	throw_faiss("virtual void faiss::Index::range_search(...) const", "faiss/Index.cpp", "range search not implemented");
}
void IndexBase::range_search_mapped(int64_t, const float *, float, const mvs_search_params *, const int64_t *, RangeResult &, hipStream_t) {
	throw_faiss("virtual void faiss::Index::range_search(...) const", "faiss/Index.cpp", "range search not implemented");
}

int64_t IndexBase::remove_ids(const mvs_search_params *, const int64_t *, RemoveMarks *) {
	throw_faiss("virtual size_t faiss::Index::remove_ids(const faiss::IDSelector&)", "faiss/Index.cpp", "remove_ids not implemented for this type of index");
}
void IndexBase::tie_emit(const int *, int, const float *, const float *, int64_t, const mvs_search_params *, const int64_t *, float *,
                         int64_t *, int *, hipStream_t) {
	throw_faiss("mvs::IndexBase::tie_emit", __FILE__, "not an IVF row shard");
}
void IndexBase::begin_kernel_timing(hipStream_t st) {
	if (!timing_enabled)
		return;
	hipEvent_t a, b;
	MVS_HIP(hipEventCreate(&a));
	MVS_HIP(hipEventCreate(&b));
	timing_events.emplace_back(a, b);
	MVS_HIP(hipEventRecord(a, st));
}
void IndexBase::end_kernel_timing(hipStream_t st) {
	if (!timing_enabled)
		return;
	MVS_HIP(hipEventRecord(timing_events.back().second, st));
}
// what the search's dominant launch was (mvs_index_last_kernel_info); the timing fields are resolve_kernel_timing's
void IndexBase::set_kinfo(const char *name, double flops, double bytes, int grid, int block, int lds_bytes, int nsplit) {
	snprintf(kinfo.name, sizeof kinfo.name, "%s", name);
	kinfo.flops = flops;
	kinfo.bytes = bytes;
	kinfo.grid = grid;
	kinfo.block = block;
	kinfo.lds_bytes = lds_bytes;
	kinfo.nsplit = nsplit;
}
void IndexBase::resolve_kernel_timing(int *count, double *total_ms) {
	for (auto &p : timing_events) {
		MVS_HIP(hipEventSynchronize(p.second));
		float ms = 0.f;
		MVS_HIP(hipEventElapsedTime(&ms, p.first, p.second));
		timing_total_ms += ms;
		timing_count++;
		kinfo.last_ms = ms;
		(void)hipEventDestroy(p.first);
		(void)hipEventDestroy(p.second);
	}
	timing_events.clear();
	*count = timing_count;
	*total_ms = timing_total_ms;
}

// ------------------------------------------------------------------------------------------ selector

SelectorDev SelectorHolder::upload(const mvs_search_params *p, const IdDomain &dom, hipStream_t st) {
	SelectorDev s;
	memset(&s, 0, sizeof s);
	if (!p || p->sel_kind == MVS_SEL_NONE)
		return s;
	if (p->sel_kind == MVS_SEL_PROGRAM) // (csrc/selector_lower.hip: evaluated over `dom`, lowered to one of the two kinds below)
		return upload_program(p, dom, st);
	s.kind = p->sel_kind;
	if (p->sel_kind == MVS_SEL_BITMAP) {
		// faiss::IDSelectorBitmap(n_bytes, bitmap): src/faiss_extension.cpp:959
		buf.reserve((size_t)std::max<int64_t>(p->sel_n, 1));
		if (p->sel_n > 0)
			MVS_HIP(hipMemcpyAsync(buf.p, p->sel_data, (size_t)p->sel_n, hipMemcpyHostToDevice, st));
		s.bitmap = (const uint8_t *)buf.p;
		s.nbytes = p->sel_n;
	} else if (p->sel_kind == MVS_SEL_BATCH) {
		// faiss::IDSelectorBatch(n, ids): bloom filter + hash set == set membership; sorted array + bisect here
		sorted.assign((const int64_t *)p->sel_data, (const int64_t *)p->sel_data + p->sel_n);
		std::sort(sorted.begin(), sorted.end());
		buf.reserve(std::max<size_t>(sorted.size() * sizeof(int64_t), 8));
		if (!sorted.empty())
			MVS_HIP(hipMemcpyAsync(buf.p, sorted.data(), sorted.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
		s.sorted_ids = (const int64_t *)buf.p;
		s.nids = (int64_t)sorted.size();
	} else {
		throw_faiss("mvs::SelectorHolder::upload", __FILE__, "unknown selector kind %d", p->sel_kind);
	}
	return s;
}

// ------------------------------------------------------------------------------------------ Flat

FlatIndex::FlatIndex(int d_, int metric_) : IndexBase(MVS_KIND_FLAT, d_, metric_) {
	if (metric != METRIC_L2 && metric != METRIC_IP && !metric_is_extra(metric))
		throw_faiss("mvs::FlatIndex::FlatIndex", __FILE__, "metric type %d is not a faiss::MetricType the glue registers",
		            metric);
	geom = flat_geom_for(d);
	bf = DevRowStore((size_t)2 * geom.dp * sizeof(unsigned short), 0, 64);
	h1 = DevRowStore((size_t)collect_store_dims(d) * sizeof(unsigned short), sizeof(float), 192);
	i8 = DevRowStore(128, sizeof(int), 256);
	is_trained = true;
	if (const char *e = getenv("MVS_LAZY_ADDS")) // (same-box A/B of the ingest staging through host/boundary_driver, which sets no options)
		lazy_adds = atoi(e) != 0;
}
FlatIndex::~FlatIndex() {
	delete shadow;
	shadow = nullptr;
	(void)hipSetDevice(device);
	if (stream)
		(void)hipStreamSynchronize(stream);
	reap_retired(true);
	// (the row stores, the derived stores, the workspaces and the pinned reports free themselves after this body and before ~IndexBase destroys the stream)
}

void FlatIndex::drop_bf16_rows() {
	bf.drop();
	h1.drop();
	mu_h1.release();
	drop_i8();
	i8_state = 0; // (the next build decides again)
	d_outl.release();
	h1_outliers = 0;
	d_max_norm_bits.release();
}
// [16] zero words, on first use
void FlatIndex::ensure_max_norm_bits(hipStream_t st) {
	if (d_max_norm_bits)
		return;
	d_max_norm_bits = DevBlock<unsigned>(16);
	MVS_HIP(hipMemsetAsync(d_max_norm_bits.get(), 0, 64, st));
}

// rows [bf.n, ntotal) of the f32 store -> bf16 hi/lo (+ running maximum of the squared norms); derived data, so add(),
// clone() and to_device() never have to know about it
void FlatIndex::ensure_bf16_rows(hipStream_t st) {
	if (bf.n == ntotal && vecs_bf())
		return;
	if (ntotal > bf.cap || !vecs_bf())
		bf.grow(std::max<int64_t>(cap, ntotal), st);
	ensure_max_norm_bits(st);
	launch_rows_to_bf16(geom, vecs(), bf.n, ntotal - bf.n, vecs_bf(), norms(), d_max_norm_bits.get(), st);
	bf.n = ntotal;
}

void FlatIndex::reset() {
	if (pend_slot >= 0) { // (staged rows die with the index's contents: the slot goes back to the ring unused)
		pend_rows = 0;
		flush_adds();
	}
	ntotal = 0;
	++mut_gen; // (rows change in place from here on: a shadow clustering of the old rows must not answer -- ADVICE r5)
	drop_bf16_rows();
	drop_shadow();
	if (shadow_state == 1)
		shadow_state = 0;
}

// faiss::IndexFlatCodes::remove_ids: row r goes iff label_offset + r (under IDMap: id_map[r]) is a member; the survivors keep their order and
// are renumbered 0 .. ntotal'-1.  Out of place (csrc/remove_ids.hip): a fresh store of the same capacity, the old one retired
int64_t FlatIndex::remove_ids(const mvs_search_params *sel, const int64_t *d_idmap, RemoveMarks *marks) {
	use_device();
	check_remove_selector(sel);
	flush_adds();
	if (ntotal <= 0)
		return 0;
	if (have_last_search) // (a search enqueued on the caller's stream may still read the rows and the selector buffer)
		stream_wait(stream, last_search_stream);
	// (MVS_REMOVE_PROFILE=1: where the call's time goes, on stderr -- tools/remove_bench.py)
	const bool prof = getenv("MVS_REMOVE_PROFILE") != nullptr;
	auto t_prev = std::chrono::steady_clock::now();
	auto lap = [&](const char *what) {
		if (!prof)
			return;
		(void)hipStreamSynchronize(stream);
		const auto t = std::chrono::steady_clock::now();
		fprintf(stderr, "removeprofile\tFlat %s: %.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count());
		t_prev = t;
	};
	RemoveMarks own;
	RemoveMarks &m = marks ? *marks : own;
	const SelectorDev sd = selector.upload(sel, IdDomain::rows(label_offset, ntotal, d_idmap), stream);
	lap("selector sort + upload");
	const int64_t nkeep = remove_mark(m, sd, d_idmap, label_offset, ntotal, stream);
	lap("mark + scan");
	if (nkeep == ntotal)
		return 0; // (no member: nothing is touched, no derived store invalidated)
	DevBlock<float> nv, nn;
	alloc_rows(cap, nv, nn); // (before anything changes: a failure leaves the index as it was)
	lap("allocation");
	try {
		launch_remove_compact_flat(geom, vecs(), norms(), m, nv.get(), nn.get(), stream);
		// (waited for here, 2 ms at 10 M rows: the derived stores are freed next, and hipFree waits for the whole device anyway)
		MVS_HIP(hipStreamSynchronize(stream));
		lap("compaction");
	} catch (...) {
		(void)hipStreamSynchronize(stream); // (nv and nn are freed on the way out: nothing may still write to them)
		throw;
	}
	replace_rows(stream, std::move(nv), std::move(nn));
	const int64_t removed = ntotal - nkeep;
	ntotal = nkeep;
	// everything derived from the rows goes, as after reset() and adding the survivors again: the bf16 hi/lo, h1 and int8 stores with the
	// outlier list and the norm maxima (drop_bf16_rows), the shadow clustering, what earlier searches learnt about the data
	++mut_gen;
	drop_bf16_rows();
	drop_shadow();
	if (shadow_state == 1)
		shadow_state = 0;
	have_last_search = false;
	cl_cap_hint = 0;
	cl_est_per_query = 0;
	cl_fpitch = 256;
	cl_fbucket_off = false;
	cl_skip = cl_skip_len = 0;
	lap("derived stores dropped");
	own.flags.release(), own.dest.release(), own.temp.release();
	lap("marks freed");
	return removed;
}

void FlatIndex::copy_rows_to_host(float *out) {
	use_device();
	flush_adds();
	MVS_HIP(hipStreamSynchronize(stream));
	if (ntotal <= 0)
		return;
	std::vector<float> tmp((size_t)ntotal * geom.dp);
	MVS_HIP(hipMemcpy(tmp.data(), vecs(), tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
	for (int64_t r = 0; r < ntotal; ++r) {
		const float *s = &tmp[(size_t)r * geom.dp];
		for (int kk = 0; kk < d; ++kk) {
			int src = kk;
			if (geom.pair_interleaved) { // stored [k0,k2,k1,k3] (bit 4 of r clear) or [k1,k3,k0,k2]
				static const int pos0[4] = {0, 2, 1, 3}, pos1[4] = {2, 0, 3, 1};
				src = (kk & ~3) + (((r >> 4) & 1) ? pos1[kk & 3] : pos0[kk & 3]);
			}
			out[(size_t)r * d + kk] = s[src];
		}
	}
}

void FlatIndex::grow(int64_t need, hipStream_t st) {
	if (need <= cap)
		return;
	// doubling for chunked ingest (every growth re-allocates and copies all rows: 19 growths by 1.5 were 35-49 ms of a 10 M row
	// ingest's 400), exactly `need` for an add larger than that.  Round 6: by FOUR while the store is below 2 GB (a growth costs ~ 3 ms of
	// hipMalloc under faiss_lock whatever its size: 14 of them were 39 of a 10 M-row ingest's 275 ms; 288 GB of HBM can afford the slack)
	const int64_t row_bytes = (int64_t)geom.dp * 4;
	const int64_t nc = std::max<int64_t>(need, (cap * row_bytes < ((int64_t)2 << 30) ? 4 : 2) * cap + 4096);
	DevBlock<float> nv, nn;
	alloc_rows(nc, nv, nn);
	// (rows staged but not flushed yet -- pend_rows -- are not on the device: only what is there is copied)
	const int64_t have = ntotal - pend_rows;
	if (have > 0) {
		MVS_HIP(hipMemcpyAsync(nv.get(), vecs(), (size_t)have * geom.dp * sizeof(float), hipMemcpyDeviceToDevice, st));
		MVS_HIP(hipMemcpyAsync(nn.get(), norms(), (size_t)have * sizeof(float), hipMemcpyDeviceToDevice, st));
	}
	// round 6: the old buffers are freed when the copy out of them has finished -- checked at the next growth, flush or reader, never
	// waited for here (round 5: a stream synchronisation + two hipFree per growth, 4 ms each, 10 % of a 10 M-row ingest under faiss_lock)
	replace_rows(st, std::move(nv), std::move(nn));
	cap = nc;
}
void FlatIndex::alloc_rows(int64_t rows, DevBlock<float> &nv, DevBlock<float> &nn) const {
	// +64 floats: the LDS-DMA staging reads whole 64-float pieces and may run past the last row; the prefilter stages norms past the end
	nv = DevBlock<float>((size_t)rows * geom.dp + 64);
	nn = DevBlock<float>((size_t)rows + 64);
}
void FlatIndex::replace_rows(hipStream_t st, DevBlock<float> &&nv, DevBlock<float> &&nn) {
	// (not reaped here: hipFree waits for the whole device -- during an ingest that is a stall under faiss_lock; readers reap)
	if (vecs_ || norms_) {
		retired.reserve(retired.size() + 1);
		hipEvent_t done;
		MVS_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
		MVS_HIP(hipEventRecord(done, st));
		retired.push_back(Retired {std::move(vecs_), std::move(norms_), done});
	}
	vecs_ = std::move(nv);
	norms_ = std::move(nn);
}
void FlatIndex::reap_retired(bool wait) {
	for (size_t i = 0; i < retired.size();) {
		Retired &r = retired[i];
		if (wait)
			(void)hipEventSynchronize(r.done);
		else if (hipEventQuery(r.done) != hipSuccess) {
			++i;
			continue;
		}
		(void)hipEventDestroy(r.done);
		retired.erase(retired.begin() + (long)i); // (frees the pair)
	}
}
// Ingest staging (round 6).  The glue adds <= 2048 rows per call under faiss_lock
// (src/faiss_extension.cpp:475-547); round 5 paid a staging copy, an H2D copy, two kernel launches and an event record per call
// (39-60 us per 1 MB: 13 GB/s of a 57 GB/s link).  Now a call only copies its rows behind the previous call's in the current pinned slot
// (8 MB); the H2D copy, pack_rows and the norms run ONCE per slot -- when it is full, or when anything wants to read the rows.
bool FlatIndex::flush_adds() {
	if (pend_slot < 0)
		return false;
	TraceRange tr("mvs:stage_rows (H2D + pack_rows + norms of one pinned slot)");
	const bool sent = pend_rows > 0;
	if (pend_rows > 0) {
		ws_add.reserve((size_t)2 * PinnedRing::SLOT_BYTES);
		float *raw = (float *)((char *)ws_add.p + (size_t)add_flip * PinnedRing::SLOT_BYTES);
		add_flip ^= 1;
		MVS_HIP(hipMemcpyAsync(raw, add_ring.buf[pend_slot], pend_bytes, hipMemcpyHostToDevice, stream));
		add_ring.release(pend_slot, stream);
		launch_pack_rows(geom, raw, pend_rows, vecs() + (size_t)pend_row0 * geom.dp, pend_row0, stream);
		launch_query_norms(raw, pend_rows, d, norms() + pend_row0, stream);
		++add_flushes;
	}
	pend_slot = -1;
	pend_bytes = 0;
	pend_rows = 0;
	return sent;
}

// faiss::IndexFlatCodes::add: append n*d floats  (src/faiss_extension.cpp:512,609)
void FlatIndex::add(int64_t n, const float *x) {
	use_device();
	if (n <= 0)
		return;
	if (ntotal + n > (int64_t)0x7fffffff - 1024)
		throw_faiss("mvs::FlatIndex::add", __FILE__, "a single-device shard holds at most 2^31 rows");
	grow(ntotal + n, stream);
	const size_t nbytes = (size_t)n * d * sizeof(float);
	if (lazy_adds && nbytes <= PinnedRing::SLOT_BYTES / 2) {
		// a DataChunk-sized add: behind the rows already staged in the current slot; the device side runs once per slot (flush_adds)
		if (pend_slot >= 0 && pend_bytes + nbytes > PinnedRing::SLOT_BYTES)
			flush_adds();
		if (pend_slot < 0) {
			pend_slot = add_ring.acquire(PinnedRing::SLOT_BYTES);
			pend_bytes = 0, pend_rows = 0, pend_row0 = ntotal;
		}
		stage_copy_mt((char *)add_ring.buf[pend_slot] + pend_bytes, x, nbytes);
		pend_bytes += nbytes;
		pend_rows += n;
		ntotal += n;
		if (pend_bytes + nbytes > PinnedRing::SLOT_BYTES) // (no room for another chunk of this size: the copy engine takes the slot
			flush_adds();                                 // now, while the callers stage the next one)
		return;
	}
	flush_adds();
	// pinned staging in slots of <= SLOT_BYTES (the caller's buffer is free again when we return); each slot is
	// copied H2D into a raw device buffer and re-laid out into the storage format by pack_rows
	const int64_t rows_per_slot = std::max<int64_t>(1, (int64_t)PinnedRing::SLOT_BYTES / ((int64_t)d * 4));
	ws_add.reserve((size_t)2 * PinnedRing::SLOT_BYTES);
	for (int64_t r0 = 0; r0 < n; r0 += rows_per_slot) {
		const int64_t nr = std::min(rows_per_slot, n - r0);
		const size_t bytes = (size_t)nr * d * sizeof(float);
		const int slot = add_ring.acquire(bytes);
		stage_copy_mt(add_ring.buf[slot], x + r0 * d, bytes);
		float *raw = (float *)((char *)ws_add.p + (size_t)add_flip * PinnedRing::SLOT_BYTES);
		add_flip ^= 1;
		MVS_HIP(hipMemcpyAsync(raw, add_ring.buf[slot], bytes, hipMemcpyHostToDevice, stream));
		add_ring.release(slot, stream);
		launch_pack_rows(geom, raw, nr, vecs() + (size_t)(ntotal + r0) * geom.dp, ntotal + r0, stream);
		launch_query_norms(raw, nr, d, norms() + ntotal + r0, stream);
	}
	ntotal += n;
}

void FlatIndex::add_device(int64_t n, const float *d_x, hipStream_t st) {
	use_device();
	if (n <= 0)
		return;
	flush_adds();
	stream_wait(st, stream); // earlier host-API adds live on our own stream
	grow(ntotal + n, st);
	launch_pack_rows(geom, d_x, n, vecs() + (size_t)ntotal * geom.dp, ntotal, st);
	launch_query_norms(d_x, n, d, norms() + ntotal, st);
	stream_wait(stream, st); // later host-API calls see these rows
	ntotal += n;
}

__global__ void fill_results_kernel(float *D, long long *I, long long total, float v) {
	long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < total) {
		D[i] = v;
		I[i] = -1;
	}
}

// L1, Linf, Lp, Canberra, BrayCurtis, JensenShannon, Jaccard [IndexFlat::search -> knn_extra_metrics,
// faiss/utils/extra_distances.cpp]: per-pair value on the LDS-staged flat_direct kernel (one instance per metric), the
// partial lists merged under the metric's order.  A cold path of the reference (the glue only forwards the metric
// name); no MFMA shape exists for these, the kernel is VALU-bound (|x-y| chains) or transcendental-bound (Lp, JS).
// Jaccard is a similarity: CMin lists like inner product, exact ties at the k-th score resolved in the pure order.
void FlatIndex::search_extra_metric(const FlatSearchRequest &r) {
	if (r.kk > flat_direct_max_k())
		throw_faiss("mvs::FlatIndex::search", __FILE__, "k = %lld exceeds the supported maximum %lld", (long long)r.kk,
		            (long long)flat_direct_max_k());
	memset(&kinfo, 0, sizeof kinfo);
	exact_direct(r); // (no tie flags: the merge under metric_order(metric) is the whole tail)
}

// ---- host driver of the Flat search (DESIGN.md 3.1 "Host driver") ---------------------------------------------------------------------
// IndexFlat::search dispatch (faiss/IndexFlat.cpp, utils/distances.cpp):
//   sel || nq < 20 -> per-pair arithmetic (flat_direct.hip); else BLAS-branch arithmetic (flat_mfma.hip)
// ENTRY: staged adds, retired buffers and last_search_stream are touched here and nowhere else in the driver
void FlatIndex::search_flat(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I,
                            const mvs_search_params *params, const int64_t *d_idmap, hipStream_t st) {
	use_device();
	TraceRange tr("mvs:flat_search");
	if (!retired.empty())
		reap_retired(false);
	if (flush_adds()) // (rows staged by add() reach the device before anything reads them)
		stream_wait(st, stream);
	if (k <= 0)
		throw_faiss("virtual void faiss::IndexFlat::search(...) const", "faiss/IndexFlat.cpp", "Error: 'k > 0' failed");
	if (nq <= 0)
		return;
	if (ntotal == 0) {
		const long long total = (long long)nq * k;
		hipLaunchKernelGGL(fill_results_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_D,
		                   (long long *)d_I, total, metric_order(metric) == METRIC_L2 ? FLT_MAX : -FLT_MAX);
		return;
	}
	// the scratch buffers below are shared by all searches of this index: order this call after the last one
	if (have_last_search) // (a null last_search_stream is HIP's NULL stream, a legitimate caller stream)
		stream_wait(st, last_search_stream);
	last_search_stream = st;
	have_last_search = true;
	FlatSearchRequest top {};
	top.nq = nq, top.d_x = d_x, top.k_user = top.kk = k, top.D = d_D, top.I = d_I, top.params = params, top.d_idmap = d_idmap, top.st = st;
	top.out_map = raw_rows ? nullptr : d_idmap, top.out_off = raw_rows ? 0 : label_offset;
	top.pair_branch = nq < 20;
	if (metric_is_extra(metric))
		search_extra_metric(top);
	else
		tie_wrapped_search(top);
}

// TIE WRAPPER.  Inner product, exact ties at the k-th score: FAISS's CMin heap keeps/evicts equal scores by
// arrival order.  The kernels keep the pure order (score desc, row id asc) -- a function of the data alone, so
// it merges across splits -- with ONE extra entry per list; the merge flags the queries whose k-th and (k+1)-th
// scores are bit-equal and resolve_ip_ties() replays the heap's outcome for those (usually none).
// A re-run of unproven queries enters here (rerun_unproven): its own flags, after the outer pass has consumed those of the batch.
void FlatIndex::tie_wrapped_search(const FlatSearchRequest &rq) {
	std::optional<QuietScope> hush; // (a quiet pass: kernel timing off, kinfo put back -- on every exit)
	if (rq.quiet)
		hush.emplace(*this);
	const int64_t nq = rq.nq, k = rq.k_user;
	// (k >= 100: FAISS's reservoir instead of its heap -- resolve_ip_ties replays that; any kernel may serve the k + 1 search)
	const bool tie_detect = metric == METRIC_IP && ip_exact_ties && !raw_rows && ntotal > k &&
	                        (k + 1 <= flat_mfma_max_k(geom) || (k >= 100 && k + 1 <= std::min(flat_direct_max_k(), reservoir_replay_max_k())));
	if (!tie_detect) {
		route(rq);
		return;
	}
	FlatSearchRequest in = rq;
	in.kk = k + 1;
	// raw candidate lists of the flagged queries: kk entries each, or the prefilter's kk + margin (search_prefilter)
	const size_t kflag = (size_t)(in.kk + std::max<int64_t>(16, in.kk / 2));
	ws_flag.reserve(16 + (size_t)nq * 4 + (size_t)nq * kflag * 8);
	TieFlags fl;
	fl.count = (int *)ws_flag.p;
	fl.query = fl.count + 4;
	fl.val = (float *)(fl.query + nq);
	fl.row = (int *)(fl.val + (size_t)nq * kflag);
	MVS_HIP(hipMemsetAsync(fl.count, 0, sizeof(int), rq.st));
	in.flags = &fl;
	route(in);
}

// ROUTE: which filter or exact kernel takes the pass.
// Inner product + selector: FAISS's per-pair fvec_inner_product is the k-ordered chain the MFMA computes, so the
// filtered search -- the reference's signature feature, on its default metric -- stays on the fused kernel, which
// masks the rejected rows in its epilogue.  (L2 + selector is Sum (x-y)^2 per pair: packed scan kernel.)
// The same identity covers small inner-product batches (nq < 20, FAISS's per-pair branch): from 8 queries on the
// MFMA kernel beats the per-pair kernels even with a mostly empty 128-query block.
// (queries re-run for the prefilter belong to a batch FAISS sends down its BLAS branch, however few they are: pair_branch)
void FlatIndex::route(const FlatSearchRequest &r) {
	const int64_t nq = r.nq, k = r.kk, mfma_kmax = flat_mfma_max_k(geom);
	const bool has_sel = r.has_sel(), small_batch = r.pair_branch, forced = force_direct || force_staged;
	const bool ip_on_mfma = metric == METRIC_IP && (has_sel || small_batch) && nq >= 8 &&
	                        k <= (has_sel ? flat_mfma_max_k_lds(geom) : mfma_kmax) && !forced;
	const bool direct = ((has_sel || small_batch) && !ip_on_mfma) || k > mfma_kmax || force_direct;
	memset(&kinfo, 0, sizeof kinfo);
	// The coarse filter FIRST for
	//   * L2 + selector, or a small batch (FAISS's per-pair branch) on a large database: it masks by the selector and re-scores its
	//     candidates with the per-pair arithmetic FAISS uses there (csrc/flat_collect.hip); same results as the packed scan / staged kernels
	//     (inner product + selector beyond the fused kernel's LDS lists -- k in the dozens and above -- likewise, instead of the per-pair scan);
	//   * (round 6) lists beyond the fused kernel's: the coarse filter's big-list path (CollectPlan::bigk, csrc/flat_coarse.hip)
	const bool filter_first = !forced && (((has_sel && (metric == METRIC_L2 || !ip_on_mfma)) || small_batch) || (k > mfma_kmax && !has_sel && !small_batch));
	if (filter_first && search_prefilter(r))
		return;
	if (!direct) {
		// bf16 coarse filter / bf16x3 prefilter + exact re-scoring (csrc/flat_coarse.hip; same results), else the fused f32 kernel.
		// (a small inner-product batch on the MFMA kernel has been declined by the filter above and is asked again here: DESIGN.md 3.1)
		if (!search_prefilter(r))
			exact_mfma(r);
		return;
	}
	if (k > flat_direct_max_k())
		throw_faiss("mvs::FlatIndex::search", __FILE__, "k = %lld exceeds the supported maximum %lld",
		            (long long)k, (long long)flat_direct_max_k());
	// 1-4 queries are pure streaming: the LDS-staged kernel (coalesced tiles, 1 or 4 chains per thread) reaches
	// 3.2 TB/s there, the thread-per-row scan 1.6; from ~8 queries on the packed scan wins (3x at nq = 2000)
	if ((metric != METRIC_L2 || has_sel || small_batch) && !force_staged && nq > 4 && ivf_scan_supported(geom.dp, k))
		exact_pair_scan(r);
	else
		exact_direct(r);
}

void FlatIndex::reserve_partials(const FlatSearchRequest &r, int64_t nparts) {
	ws_pd.reserve((size_t)nparts * r.nq * r.kk * sizeof(float));
	ws_pi.reserve((size_t)nparts * r.nq * r.kk * sizeof(int32_t));
	ws_gthr.reserve((size_t)r.nq * ((r.kk + 15) / 16 * 16) * sizeof(unsigned) + 64); // shared threshold slots
}
void FlatIndex::finish_exact(const FlatSearchRequest &r, const ExactLaunch &x) {
	launch_merge_partials(metric_order(metric), (const float *)ws_pd.p, (const int32_t *)ws_pi.p, x.nparts, r.nq, r.kk, r.out_map, r.out_off, r.D,
	                      r.I, r.st, r.k_user, r.flags);
	if (r.flags)
		resolve_ip_ties(r.nq, r.d_x, r.k_user, *r.flags, x.sel, r.d_idmap, r.D, r.I, r.st);
	set_kinfo(x.name, x.flops, x.bytes, x.grid, 256, x.lds_bytes, x.nparts);
}

// per-pair arithmetic (exhaustive_L2sqr_seq / exhaustive_inner_product_seq): packed-fp32 scan kernel of csrc/ivf_scan.hip in grid mode
void FlatIndex::exact_pair_scan(const FlatSearchRequest &r) {
	const int64_t nq = r.nq, k = r.kk;
	hipStream_t st = r.st;
	const int ngroups = (int)((nq + 19) / 20);
	const int64_t ntiles = (ntotal + 255) / 256;
	int64_t nsplit = std::max<int64_t>(1, std::min<int64_t>(4096 / ngroups, ntiles / 4));
	while (nsplit > 1 && (size_t)(nsplit + 1) * k * 8 > 150 * 1024) // the merge kernel keeps nsplit*k candidates in LDS
		nsplit /= 2;
	const int64_t split_rows = (ntiles + nsplit - 1) / nsplit * 256;
	nsplit = (ntotal + split_rows - 1) / split_rows;
	ws_q.reserve((size_t)nq * geom.dp * sizeof(float));
	launch_pad_rows(r.d_x, nq, d, (float *)ws_q.p, geom.dp, st);
	reserve_partials(r, nsplit);
	ws_xi.reserve(ivf_scan_query_pack_bytes(geom.dp, ngroups));
	SelectorDev sel = selector.upload(r.params, sel_domain(r.d_idmap), st);
	begin_kernel_timing(st);
	launch_init_slots((unsigned *)ws_gthr.p, nq, k, metric, st);
	launch_pair_scan(geom.dp, geom.pair_interleaved, metric, (const float *)ws_q.p, nq, vecs(), ntotal, k, (int)nsplit,
	                 split_rows, sel, r.d_idmap, (float *)ws_pd.p, (int32_t *)ws_pi.p, (unsigned *)ws_gthr.p,
	                 (float *)ws_xi.p, st);
	end_kernel_timing(st);
	finish_exact(r, {sel, (int)nsplit, (int)(nsplit * ngroups), (int)ivf_scan_lds_bytes(k), "flat_pair_scan (ivf_scan_kernel)",
	                 2.0 * (double)nq * (double)ntotal * d * (metric == METRIC_L2 ? 1.5 : 1.0), (double)ngroups * (double)ntotal * geom.dp * 4.0});
}

// the LDS-staged kernel (csrc/flat_direct.hip): per-pair arithmetic; the BLAS-branch value (formula) when FAISS would have used sgemm
// (nq >= 20, no selector) but k is too large for the fused kernel's LDS lists; one instance per extra metric (search_extra_metric)
void FlatIndex::exact_direct(const FlatSearchRequest &r) {
	const int64_t nq = r.nq, k = r.kk;
	hipStream_t st = r.st;
	const bool extra = metric_is_extra(metric), formula = metric == METRIC_L2 && !r.has_sel() && !r.pair_branch;
	FlatDB db {vecs(), norms(), ntotal};
	DirectPlan p = extra ? plan_flat_direct_extra(geom, nq, ntotal, k) : plan_flat_direct(geom, nq, ntotal, k);
	const int64_t ngroups = (nq + p.qgroup - 1) / p.qgroup, nq_pad = ngroups * p.qgroup;
	ws_q.reserve((size_t)nq_pad * geom.dp * sizeof(float));
	MVS_HIP(hipMemsetAsync(ws_q.p, 0, (size_t)nq_pad * geom.dp * sizeof(float), st));
	launch_pad_rows(r.d_x, nq, d, (float *)ws_q.p, geom.dp, st);
	float *qn = nullptr;
	if (formula) {
		ws_qn.reserve((size_t)nq * sizeof(float));
		qn = (float *)ws_qn.p;
		launch_row_norms((const float *)ws_q.p, nq, geom.dp, qn, st);
	}
	reserve_partials(r, p.nsplit); // (the 4 per-wave lists are merged inside the workgroup)
	SelectorDev sel = selector.upload(r.params, sel_domain(r.d_idmap), st);
	begin_kernel_timing(st);
	launch_init_slots((unsigned *)ws_gthr.p, nq, k, metric_order(metric), st);
	if (extra)
		launch_flat_direct_extra(geom, p, metric, metric_arg, d, (const float *)ws_q.p, nq, db, k, sel, r.d_idmap,
		                         (float *)ws_pd.p, (int32_t *)ws_pi.p, (unsigned *)ws_gthr.p, st);
	else
		launch_flat_direct_ex(geom, p, metric, formula, (const float *)ws_q.p, qn, nq, db, k, sel, r.d_idmap,
		                      (float *)ws_pd.p, (int32_t *)ws_pi.p, (unsigned *)ws_gthr.p, st);
	end_kernel_timing(st);
	char name[64] = "flat_direct_kernel";
	if (extra)
		snprintf(name, sizeof name, "flat_direct_kernel (metric %d)", metric);
	const double flops = extra ? 3.0 * (double)nq * (double)ntotal * d : 2.0 * (double)nq * (double)ntotal * d * (metric == METRIC_L2 && !formula ? 1.5 : 1.0);
	finish_exact(r, {sel, p.nsplit, p.grid, (int)p.lds_bytes, name, flops, (double)ngroups * (double)ntotal * geom.dp * 4.0});
}

// the fused f32 MFMA kernel (csrc/flat_mfma.hip): BLAS-branch arithmetic.  (Timing begins before the selector upload and the kernel
// initialises its threshold slots itself -- unlike the two branches above.)
void FlatIndex::exact_mfma(const FlatSearchRequest &r) {
	const int64_t nq = r.nq, k = r.kk;
	hipStream_t st = r.st;
	FlatDB db {vecs(), norms(), ntotal};
	FlatSearchPlan p = plan_flat_mfma(geom, nq, ntotal, k);
	ws_q.reserve(qfrag_floats(geom, nq) * sizeof(float));
	ws_qn.reserve((size_t)nq * sizeof(float));
	launch_pack_queries(geom, r.d_x, nq, (float *)ws_q.p, (float *)ws_qn.p, st);
	reserve_partials(r, p.nsplit);
	begin_kernel_timing(st);
	SelectorDev sel = selector.upload(r.params, sel_domain(r.d_idmap), st);
	launch_flat_mfma(geom, p, metric, (const float *)ws_q.p, (const float *)ws_qn.p, nq, db, k, (float *)ws_pd.p,
	                 (int32_t *)ws_pi.p, (unsigned *)ws_gthr.p, st, &sel, r.d_idmap);
	end_kernel_timing(st);
	finish_exact(r, {sel, p.nsplit, p.grid, (int)p.lds_bytes, "flat_mfma_kernel", 2.0 * (double)nq * (double)ntotal * d,
	                 (double)ntotal * d * 4.0 + (double)nq * d * 4.0 + (double)nq * r.k_user * 12.0});
}

// ---- shadow clustering of a Flat L2 index (round 5) ------------------------------------------------------------------
// The coarse filter's error bound scales with ||x - mu|| ||y - mu|| for ONE centre mu.  Rows that form clusters far from each other
// (embeddings; the C3 mixture: 1024 centres of norm^2 ~ 128, neighbours at distance^2 ~ 2.6) leave 2E larger than the spread of
// distances inside the query's cluster: the whole cluster is admitted (9 764 candidates per query, 45.6 ms per 10k batch against
// 17.3 on uniform rows).  The cure is the IVF index's per-list centring -- so the Flat index keeps one: k-means over its rows
// (sqrt(N) lists), the rows list by list as bf16 residuals, and a large batch runs
//   1. the IVF coarse filter over the nprobe nearest lists (C3's kernels), candidates re-scored with THIS index's arithmetic
//      ((xn + yn) - 2 ip on the original rows, ties by row number) -- the result is exact IF no other list holds a better row;
//   2. the proof, per query, that none does: every row of list j is at least ||x - c_j|| - r_j away (ivf_shadow_verify_kernel);
//   3. the queries that cannot be proven (none on clustered rows; all on uniform rows) again on the Flat kernels.
// More than a tenth of a batch unproven: the data does not cluster, the shadow is dropped for good.  false: the batch takes the normal path.
void FlatIndex::drop_shadow() {
	delete shadow;
	shadow = nullptr;
	shadow_rows = -1;
	shadow_trained_rows = 0;
	shadow_gen = 0;
}
// Build (or extend) the shadow from the rows WHERE THEY ARE (round 6; round 5 copied every row to the host, re-laid it out there, trained
// and re-added from host memory inside the first large search, and dropped the whole clustering on every add()):
//   * training sample: min(N, 256 nlist) rows at an even stride, unpacked on the device, ONE copy to the host for the k-means driver
//     (csrc/ivf.hip kmeans keeps FAISS's host-side control flow); the sample has exactly the size FAISS would subsample to;
//   * rows: unpacked in 1 M-row blocks on the device and appended through the IVF index's device add -- no host round trip;
//   * rows added to the Flat index later are APPENDED (assign + append is the IVF add): the next large search extends the shadow by
//     rows [shadow_rows, ntotal); the clustering is re-trained only after the index has doubled since it was trained;
//   * reset() (and anything else that changes rows in place) bumps mut_gen: a shadow of another generation is dropped.
bool FlatIndex::shadow_sync(hipStream_t st) {
	if (shadow && (shadow_gen != mut_gen || shadow_rows > ntotal || ntotal > 2 * std::max<int64_t>(shadow_trained_rows, 1)))
		drop_shadow();
	if (shadow && shadow_rows == ntotal)
		return true;
	const auto t0 = std::chrono::steady_clock::now();
	MVS_HIP(hipStreamSynchronize(st));
	MVS_HIP(hipStreamSynchronize(stream)); // (adds of the host API)
	const int64_t blk = (int64_t)1 << 20;
	DevBuf rows;
	bool built = false;
	if (!shadow) {
		int lg = 0;
		while (((int64_t)1 << (2 * lg + 1)) < ntotal) // nlist = the power of two nearest to sqrt(N) (N = 10 M: 4 096)
			++lg;
		const int64_t nl = std::min<int64_t>(8192, std::max<int64_t>(256, (int64_t)1 << lg));
		std::unique_ptr<IndexBase> iv(make_ivf_index(d, "IVF" + std::to_string(nl) + ",Flat", METRIC_L2));
		if (!iv)
			return false;
		iv->adopt_tuning(tune_); // (the Flat index's knobs reach its shadow and the shadow's quantizer)
		const int64_t ns = std::min<int64_t>(ntotal, nl * 256), stride = std::max<int64_t>(1, ntotal / ns);
		rows.reserve((size_t)std::max(ns, std::min(blk, ntotal)) * d * sizeof(float));
		launch_unpack_rows(geom, vecs(), 0, stride, ns, (float *)rows.p, st);
		std::vector<float> sample((size_t)ns * d);
		MVS_HIP(hipMemcpyAsync(sample.data(), rows.p, sample.size() * sizeof(float), hipMemcpyDeviceToHost, st));
		MVS_HIP(hipStreamSynchronize(st));
		iv->train(ns, sample.data());
		shadow = iv.release();
		shadow_rows = 0;
		shadow_trained_rows = ntotal;
		shadow_gen = mut_gen;
		shadow->set_timing(timing_enabled);
		use_device();
		built = true;
	} else {
		rows.reserve((size_t)std::min(blk, ntotal - shadow_rows) * d * sizeof(float));
	}
	for (int64_t r0 = shadow_rows; r0 < ntotal; r0 += blk) {
		const int64_t n = std::min(blk, ntotal - r0);
		launch_unpack_rows(geom, vecs(), r0, 1, n, (float *)rows.p, st);
		shadow->add_device(n, (const float *)rows.p, st); // (labels = row numbers: the shadow's ids continue where it stopped)
		use_device();
	}
	MVS_HIP(hipStreamSynchronize(st)); // (`rows` is freed at scope exit)
	shadow_rows = ntotal;
	const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	shadow_build_seconds += sec;
	if (built)
		++shadow_builds;
	else
		++shadow_extends;
	return true;
}
bool FlatIndex::shadow_search(const FlatSearchRequest &rq) {
	const int64_t nq = rq.nq, k = rq.k_user;
	hipStream_t st = rq.st;
	if (d % 32 != 0 || d > 128 || k > 32 || ntotal < 65536 || ntotal >= ((int64_t)1 << 31) || ntotal <= k)
		return false;
	if (!shadow_sync(st))
		return false;
	ensure_h1_rows(st); // (the proof needs the largest ||y||^2 of the rows: d_max_norm_bits[0], kept with the coarse filter's store)
	ws_qn.reserve((size_t)nq * sizeof(float));
	ws_fail.reserve(64 + (size_t)nq * sizeof(int)); // (nq >= 256: room for rerun_unproven's padding of a short fail list to 20 entries)
	int *fail_cnt = (int *)ws_fail.p, *fail_q = fail_cnt + 16;
	launch_query_norms(rq.d_x, nq, d, (float *)ws_qn.p, st);
	ensure_report();
	// (a batch the coarse quantiser's distance matrix or the pair count does not cover is served in pieces -- round 5 gave
	// the shadow up for good on the first such batch)
	const int64_t cover = shadow->flat_shadow_max_queries(shadow_nprobe);
	if (cover < 256)
		return false;
	mvs_kernel_info kacc;
	memset(&kacc, 0, sizeof kacc);
	int nf_total = 0;
	for (int64_t q0 = 0; q0 < nq; q0 += cover) {
		FlatSearchRequest piece = rq;
		piece.nq = std::min(cover, nq - q0), piece.d_x = rq.d_x + q0 * d, piece.D = rq.D + q0 * k, piece.I = rq.I + q0 * k;
		const int64_t m = piece.nq;
		MVS_HIP(hipMemsetAsync(fail_cnt, 0, sizeof(int), st));
		const int rc = shadow->flat_shadow_search(m, piece.d_x, k, (const float *)ws_qn.p + q0, piece.D, piece.I, rq.out_map, rq.out_off,
		                                          d_max_norm_bits.get(), fail_cnt, fail_q, shadow_nprobe, st);
		use_device();
		if (rc != 0) {
			// 1: this CALL's shape is not served (too few queries in the piece, ...): the batch takes the normal path, the shadow stays;
			// 2: the candidate stream / a bucket beyond their limits -- rows stored thousands of times: the shadow cannot serve this data
			if (rc == 2) {
				shadow_state = -1;
				drop_shadow();
			}
			return false;
		}
		MVS_HIP(hipMemcpyAsync(&h_report()->fail_count, fail_cnt, sizeof(int), hipMemcpyDeviceToHost, st));
		MVS_HIP(hipStreamSynchronize(st));
		const int nf = h_report()->fail_count;
		shadow_queries += m;
		shadow_unproven += nf;
		nf_total += nf;
		if (q0 == 0)
			kacc = shadow->kinfo;
		else
			kacc.flops += shadow->kinfo.flops, kacc.bytes += shadow->kinfo.bytes;
		if ((int64_t)nf * 10 > m) { // the lists of this data overlap: nothing is gained (uniform rows: every query) -- never again
			shadow_state = -1;
			drop_shadow();
			return false;
		}
		if (nf > 0) { // the unproven queries: the Flat kernels or the coarse filter decide (results overwrite theirs), never the shadow again
			rerun_unproven(piece, nf, fail_q, false);
			if (q0 + cover < nq)
				MVS_HIP(hipStreamSynchronize(st)); // (ws_fb / the fail list are reused by the next piece)
		}
	}
	kinfo = kacc;
	snprintf(kinfo.name, sizeof kinfo.name, "ivf_bf16_collect_kernel (flat shadow)");
	pf_last_fallback = nf_total;
	pf_queries_total += nq;
	pf_fallback_total += nf_total;
	return true;
}

// Tie pass of an inner-product search.  The flag count is the only host-visible decision of a search: one 4-byte
// D2H + stream sync per IP search (the search is >= 100 us of kernels).  Flagged queries are re-run through the SAME
// contraction (bit-identical scores) with the TIE epilogue, which collects per query the k smallest row ids whose
// score is >= the boundary score T; tie_resolve_kernel then applies FAISS's heap outcome (csrc/util_kernels.hip).
void FlatIndex::resolve_ip_ties(int64_t nq, const float *d_x, int64_t k, const TieFlags &fl, SelectorDev sel,
                                const int64_t *d_idmap, float *d_D, int64_t *d_I, hipStream_t st, int64_t kraw_in, const TieSource *ties) {
	ensure_report();
	MVS_HIP(hipMemcpyAsync(&h_report()->tie_flags, fl.count, sizeof(int), hipMemcpyDeviceToHost, st));
	MVS_HIP(hipStreamSynchronize(st));
	const int nf = h_report()->tie_flags;
	if (nf <= 0)
		return;
	const int64_t kraw = kraw_in > 0 ? kraw_in : k + 1; // length of the raw candidate lists the merge recorded
	if (k >= 100) {
		// FAISS collects k >= 100 results in a ReservoirTopN, not a heap (utils/distances.cpp): which of the rows tied at the k-th
		// score survive depends on the whole stream -- replayed for the flagged queries (csrc/flat_reservoir.hip)
		const size_t xf_b = ((size_t)nf * d * sizeof(float) + 255) & ~(size_t)255, t_b = ((size_t)nf * sizeof(float) + 255) & ~(size_t)255;
		const size_t ov_b = ((size_t)nf * k * sizeof(float) + 255) & ~(size_t)255, oi_b = ((size_t)nf * k * sizeof(int64_t) + 255) & ~(size_t)255;
		const int64_t F = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nf, 32768), // (flagged queries ride in grid.y)
		                                                     ((int64_t)1 << 30) / std::max<int64_t>(ntotal * 4, 1)));
		ws_tie.reserve(xf_b + t_b + 2 * ov_b + 2 * oi_b + (size_t)F * ntotal * sizeof(float) + 256);
		char *b = (char *)ws_tie.p;
		float *xf = (float *)b, *T = (float *)(b + xf_b), *ov = (float *)(b + xf_b + t_b), *Df = (float *)(b + xf_b + t_b + ov_b);
		int32_t *oi = (int32_t *)(b + xf_b + t_b + 2 * ov_b);
		int64_t *If = (int64_t *)(b + xf_b + t_b + 2 * ov_b + oi_b);
		float *scores = (float *)(b + xf_b + t_b + 2 * ov_b + 2 * oi_b);
		launch_gather_flagged(d_x, d, fl, nf, kraw, k, xf, T, st);
		for (int64_t f0 = 0; f0 < nf; f0 += F) {
			const int m = (int)std::min<int64_t>(F, nf - f0);
			launch_reservoir_replay(xf + f0 * d, m, d, vecs(), geom.dp, geom.pair_interleaved ? 1 : 0, ntotal, k, sel, d_idmap, T + f0, scores,
			                        ov + f0 * k, oi + f0 * k, st);
		}
		launch_merge_partials(METRIC_IP, ov, oi, 1, nf, k, d_idmap, label_offset, Df, If, st); // print order, labels
		launch_scatter_rows(fl.query, nf, k, Df, If, d_D, d_I, st);
		return;
	}
	const size_t xf_bytes = ((size_t)nf * d * sizeof(float) + 255) & ~(size_t)255;
	const size_t t_bytes = ((size_t)nf * sizeof(float) + 255) & ~(size_t)255;
	const size_t td_bytes = ((size_t)nf * k * sizeof(float) + 255) & ~(size_t)255;
	ws_tie.reserve(xf_bytes + t_bytes + td_bytes + (size_t)nf * k * sizeof(int64_t));
	float *xf = (float *)ws_tie.p;
	float *T = (float *)((char *)ws_tie.p + xf_bytes);
	float *tD = (float *)((char *)T + t_bytes);
	int64_t *tI = (int64_t *)((char *)tD + td_bytes);
	launch_gather_flagged(d_x, d, fl, nf, kraw, k, xf, T, st);
	(void)tD;
	CollectTieRows tr;
	tr.flag_query = fl.query, tr.T = T, tr.nf = nf, tr.k = (int)k, tr.first = tI;
	if (ties && ties->sorted) {
		tr.keys = ties->sorted, tr.seg = collect_ctl_table(ws_seg.p), tr.nq = nq;
		launch_collect_tie_rows(tr, st);
	} else if (ties && ties->bucket) { // (round 6: the bucketed finish keeps every survivor's exact key in its query's bucket)
		tr.keys = ties->bucket, tr.seg = (const int *)ties->bcount, tr.pitch = ties->bpitch;
		launch_collect_tie_rows(tr, st);
	} else
		tie_candidates(nf, xf, T, k, tI, sel, d_idmap, st);
	launch_tie_resolve(fl, nf, kraw, k, tI, d_idmap, label_offset, d_D, d_I, st);
}

__global__ void offset_rows_kernel(long long *I, long long total, long long off) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < total && I[i] >= 0)
		I[i] += off;
}
void FlatIndex::offset_rows(int64_t *d_rows, int64_t total, hipStream_t st) {
	if (total <= 0 || label_offset == 0)
		return;
	hipLaunchKernelGGL(offset_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (long long *)d_rows,
	                   (long long)total, (long long)label_offset);
}

void FlatIndex::tie_candidates(int64_t nf, const float *d_xf, const float *d_T, int64_t k, int64_t *d_rows_out,
                               SelectorDev sel, const int64_t *d_selmap, hipStream_t st) {
	use_device();
	flush_adds();
	if (nf <= 0)
		return;
	if (ntotal == 0) {
		MVS_HIP(hipMemsetAsync(d_rows_out, 0xff, (size_t)nf * k * sizeof(int64_t), st));
		return;
	}
	FlatSearchPlan p = plan_flat_mfma(geom, nf, ntotal, k);
	ws_q.reserve(qfrag_floats(geom, nf) * sizeof(float));
	launch_pack_queries(geom, d_xf, nf, (float *)ws_q.p, nullptr, st);
	ws_pd.reserve((size_t)p.nsplit * nf * k * sizeof(float));
	ws_pi.reserve((size_t)p.nsplit * nf * k * sizeof(int32_t));
	ws_gthr.reserve((size_t)nf * ((k + 15) / 16 * 16) * sizeof(unsigned) + 64);
	ws_qn.reserve((size_t)nf * k * sizeof(float)); // the merge's distance output (all 0 / FLT_MAX), unused
	FlatDB db {vecs(), norms(), ntotal};
	launch_flat_mfma_tie(geom, p, (const float *)ws_q.p, d_T, nf, db, k, (float *)ws_pd.p, (int32_t *)ws_pi.p,
	                     (unsigned *)ws_gthr.p, st, &sel, d_selmap);
	// k smallest (0, row id): the L2-ordered merge; ids come out as plain row numbers
	launch_merge_partials(METRIC_L2, (const float *)ws_pd.p, (const int32_t *)ws_pi.p, p.nsplit, nf, k, nullptr, 0,
	                      (float *)ws_qn.p, d_rows_out, st);
}

bool FlatIndex::coarse_topk(int64_t nq, const float *d_x, int64_t np, float *d_D, int64_t *d_I, hipStream_t st, bool need_matrix) {
	flush_adds();
	if (!tune().coarse_select || (metric != METRIC_L2 && metric != METRIC_IP) || nq < 20)
		return false; // (fewer than 20 queries: FAISS's per-pair branch, other arithmetic for L2)
	if (!need_matrix && metric == METRIC_L2 && tune().coarse_bf16 && coarse_bf16_supported(d, ntotal, np) && (geom.dp & 3) == 0) {
		// round 6 (csrc/coarse_bf16.hip): this index's own coarse-filter operands -- the centred bf16 store, the query fragments, ||x||^2
		// and 2E(q) of collect_query_prep_kernel -- one filter workgroup per 32 queries, one exact wavefront per query
		use_device();
		stream_wait(st, stream); // adds were enqueued on our own stream
		if (have_last_search)
			stream_wait(st, last_search_stream);
		last_search_stream = st;
		have_last_search = true;
		ensure_h1_rows(st);
		if (nq > 65536) { // (k-means assigns 10^6 training rows at once: in equal pieces of <= 64 K queries, the scratch stays that size)
			const int64_t pieces = (nq + 65535) / 65536, per = ((nq + pieces - 1) / pieces + 63) / 64 * 64; // (>= 32 K each: never a < 20-query tail)
			for (int64_t q0 = 0; q0 < nq;) {
				int64_t m = std::min<int64_t>(per, nq - q0);
				if (nq - q0 - m < 20)
					m = nq - q0;
				(void)coarse_topk(m, d_x + q0 * d, np, d_D + q0 * np, d_I + q0 * np, st, need_matrix);
				q0 += m;
			}
			return true;
		}
		ws_qn.reserve((size_t)nq * sizeof(float));
		ws_e2.reserve((size_t)((nq + 255) / 256 * 256) * sizeof(float));
		ws_pfq.reserve(collect_qfrag_bytes(geom, nq));
		ws_seg.reserve(sizeof(CollectCtl) + (size_t)2 * nq * sizeof(int));
		ws_fail.reserve(64 + (size_t)nq * sizeof(int));
		int *fail_cnt = (int *)ws_fail.p, *fail_q = fail_cnt + 16;
		MVS_HIP(hipMemsetAsync(fail_cnt, 0, sizeof(int), st));
		// (no class slots here: stride 0; queries without a finite bound come back with e2 = NaN and are computed exhaustively)
		CollectQueryPrep qp;
		qp.metric = metric, qp.x = d_x, qp.nq = nq, qp.d = d, qp.mu = mu_h1.get(), qp.max_norm_bits = d_max_norm_bits.get();
		qp.qf = ws_pfq.p, qp.qn = (float *)ws_qn.p, qp.e2 = (float *)ws_e2.p, qp.fail = {fail_cnt, fail_q};
		qp.ctl_hdr = (int *)ws_seg.p, qp.ctl_seg = collect_ctl_table(ws_seg.p);
		launch_collect_query_prep(qp, st);
		const size_t cb = (coarse_bf16_cand_bytes(nq) + 255) & ~(size_t)255, nb = ((size_t)nq * sizeof(int) + 255) & ~(size_t)255;
		const size_t lb = (coarse_bf16_cls_bytes(nq, ntotal, np) + 255) & ~(size_t)255;
		// (the exhaustive-query counter sits at the FRONT: the buffer's layout behind it changes with nq)
		const bool fresh = ws_cb16.cap < 256 + cb + nb + lb;
		ws_cb16.reserve(256 + cb + nb + lb);
		if (fresh)
			MVS_HIP(hipMemsetAsync(ws_cb16.p, 0, 256, st));
		cb16_stats_off = 0;
		char *const cbase = (char *)ws_cb16.p + 256;
		begin_kernel_timing(st);
		CoarseBf16 c;
		c.x = d_x, c.nq = nq, c.d = d, c.qf = ws_pfq.p, c.qn = (const float *)ws_qn.p, c.e2 = (const float *)ws_e2.p;
		c.yb = vecs_h1(), c.beta = beta_h1(), c.cent = vecs(), c.sdp = geom.dp, c.interleaved = geom.pair_interleaved ? 1 : 0, c.cn = norms();
		c.nlist = ntotal, c.np = np;
		c.cand = (unsigned short *)cbase, c.ccount = (int *)(cbase + cb), c.cls = (float *)(cbase + cb + nb);
		c.outD = d_D, c.outI = d_I, c.label_offset = label_offset, c.stats = (unsigned long long *)ws_cb16.p;
		launch_coarse_bf16(c, st);
		end_kernel_timing(st);
		cb16_queries += nq;
		cb16_last_nq = nq, cb16_ccount_off = 256 + cb;
		return true;
	}
	// inner product: one entry more than asked for, the merge flags boundary ties and resolve_ip_ties replays FAISS's heap
	const bool ip = metric == METRIC_IP;
	if (ip && !(ip_exact_ties && np + 1 <= flat_mfma_max_k(geom)))
		return false;
	const int64_t kk = ip ? np + 1 : np;
	if (!coarse_select_supported(ntotal, kk))
		return false;
	use_device();
	stream_wait(st, stream); // adds were enqueued on our own stream
	if (have_last_search) // the scratch buffers are shared by all searches of this index (FlatIndex::search_flat)
		stream_wait(st, last_search_stream);
	last_search_stream = st;
	have_last_search = true;
	const int64_t qchunk = std::max<int64_t>(64, std::min<int64_t>(nq, ((int64_t)512 << 20) / (ntotal * 4) / 64 * 64));
	ws_q.reserve((size_t)qchunk * ntotal * sizeof(float));
	ws_qn.reserve((size_t)nq * sizeof(float));
	ws_pd.reserve((size_t)nq * kk * sizeof(float));
	ws_pi.reserve((size_t)nq * kk * sizeof(int32_t));
	TieFlags fl = {nullptr, nullptr, nullptr, nullptr};
	if (ip) {
		const size_t kflag = (size_t)(kk + std::max<int64_t>(16, kk / 2));
		ws_flag.reserve(16 + (size_t)nq * 4 + (size_t)nq * kflag * 8);
		fl.count = (int *)ws_flag.p;
		fl.query = fl.count + 4;
		fl.val = (float *)(fl.query + nq);
		fl.row = (int *)(fl.val + (size_t)nq * kflag);
		MVS_HIP(hipMemsetAsync(fl.count, 0, sizeof(int), st));
	} else {
		launch_query_norms(d_x, nq, d, (float *)ws_qn.p, st);
	}
	begin_kernel_timing(st);
	CoarseSelect cs;
	cs.d = d, cs.cent = vecs(), cs.sdp = geom.dp, cs.interleaved = geom.pair_interleaved ? 1 : 0, cs.nlist = ntotal, cs.cn = norms();
	cs.np = kk, cs.is_l2 = ip ? 0 : 1, cs.D = (float *)ws_q.p, cs.label_offset = label_offset;
	for (int64_t q0 = 0; q0 < nq; q0 += qchunk) {
		cs.x = d_x + q0 * d, cs.nq = std::min(qchunk, nq - q0), cs.qn = (const float *)ws_qn.p + q0;
		cs.pd = (float *)ws_pd.p + q0 * kk, cs.pi = (int32_t *)ws_pi.p + q0 * kk;
		// (L2: the selection kernel writes the ordered lists itself; inner product keeps the merge -- it flags the boundary ties)
		cs.outD = ip ? nullptr : d_D + q0 * np, cs.outI = ip ? nullptr : d_I + q0 * np;
		launch_coarse_select(cs, st);
	}
	end_kernel_timing(st);
	if (ip)
		launch_merge_partials(metric, (const float *)ws_pd.p, (const int32_t *)ws_pi.p, 1, nq, kk, nullptr, label_offset, d_D, d_I, st, np, &fl);
	if (ip) {
		SelectorDev nosel;
		memset(&nosel, 0, sizeof nosel);
		resolve_ip_ties(nq, d_x, np, fl, nosel, nullptr, d_D, d_I, st);
	}
	return true;
}

void FlatIndex::search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I,
                              const mvs_search_params *params, hipStream_t st) {
	use_device();
	flush_adds();
	stream_wait(st, stream); // adds were enqueued on our own stream
	search_flat(nq, d_x, k, d_D, d_I, params, nullptr, st);
}

void FlatIndex::to_device(int new_device) {
	if (new_device == device)
		return;
	int ndev = 0;
	MVS_HIP(hipGetDeviceCount(&ndev));
	if (new_device < 0 || new_device >= ndev)
		throw_faiss("faiss::gpu::index_cpu_to_gpu", "faiss/gpu/GpuCloner.cpp", "Invalid GPU device %d", new_device);
	use_device();
	flush_adds();
	MVS_HIP(hipStreamSynchronize(stream));
	reap_retired(true);
	add_ring.drop_events();
	DevBlock<float> nv, nn;
	MVS_HIP(hipSetDevice(new_device));
	try {
		if (cap > 0) {
			alloc_rows(cap, nv, nn);
			MVS_HIP(hipMemset(nv.get(), 0, nv.cap));
			if (ntotal > 0) {
				MVS_HIP(hipMemcpyPeer(nv.get(), new_device, vecs(), device, (size_t)ntotal * geom.dp * sizeof(float)));
				MVS_HIP(hipMemcpyPeer(nn.get(), new_device, norms(), device, (size_t)ntotal * sizeof(float)));
			}
		}
	} catch (...) {
		(void)hipSetDevice(device); // (the index stays where it is)
		throw;
	}
	// the old device stays current while what lives on it goes: the rows, everything derived from them, every workspace
	MVS_HIP(hipSetDevice(device));
	vecs_ = std::move(nv);
	norms_ = std::move(nn);
	drop_bf16_rows();
	release_all();
	range_work.release(); // (the range search's hit stream, sort buffers and control block)
	selector.release();
	drop_shadow(); // (the shadow clustering lives on the old device: rebuilt on demand)
	move_stream(new_device);
}

void check_device(int dev) {
	int ndev = 0;
	MVS_HIP(hipGetDeviceCount(&ndev));
	if (dev < 0 || dev >= ndev)
		throw_faiss("faiss::gpu::index_cpu_to_gpu", "faiss/gpu/GpuCloner.cpp", "Invalid GPU device %d", dev);
}

IndexBase *FlatIndex::clone(int on_device) {
	check_device(on_device);
	use_device();
	flush_adds();
	MVS_HIP(hipStreamSynchronize(stream));
	auto *c = new FlatIndex(d, metric);
	try {
		c->to_device(on_device);
		c->use_device();
		c->grow(ntotal, c->stream);
		if (ntotal > 0) {
			MVS_HIP(hipMemcpyPeer(c->vecs(), on_device, vecs(), device, (size_t)ntotal * geom.dp * sizeof(float)));
			MVS_HIP(hipMemcpyPeer(c->norms(), on_device, norms(), device, (size_t)ntotal * sizeof(float)));
		}
		c->ntotal = ntotal;
		c->label_offset = label_offset;
	} catch (...) {
		delete c;
		throw;
	}
	return c;
}

// ------------------------------------------------------------------------------------------ IDMap

IDMapIndex::IDMapIndex(IndexBase *sub_) : IndexBase(MVS_KIND_IDMAP, sub_->d, sub_->metric), sub(sub_) {
	is_trained = sub->is_trained;
}
IDMapIndex::~IDMapIndex() {
	(void)hipSetDevice(device);
	delete sub;
}
void IDMapIndex::train(int64_t n, const float *x) {
	sub->train(n, x);
	is_trained = sub->is_trained;
}
void IDMapIndex::add(int64_t, const float *) {
	throw_faiss("virtual void faiss::IndexIDMapTemplate<IndexT>::add(faiss::idx_t, const float*)",
	            "faiss/IndexIDMap.cpp", "add does not make sense with IndexIDMap, use add_with_ids");
}
void IDMapIndex::add_device(int64_t, const float *, hipStream_t) {
	throw_faiss("virtual void faiss::IndexIDMapTemplate<IndexT>::add(faiss::idx_t, const float*)",
	            "faiss/IndexIDMap.cpp", "add does not make sense with IndexIDMap, use add_with_ids");
}
void IDMapIndex::grow_ids(int64_t need, hipStream_t st) {
	if (need <= idcap)
		return;
	// (as FlatIndex::grow; by eight while the array is below 64 MB: every growth ends in a hipFree that waits for the device)
	const int64_t nc = std::max<int64_t>(need, (idcap < ((int64_t)8 << 20) ? 8 : 2) * idcap + 4096);
	DevBlock<int64_t> ni((size_t)nc);
	flush_ids(); // (staged ids go to the old array first: the copy below carries them over)
	if (ntotal > 0)
		MVS_HIP(hipMemcpyAsync(ni.get(), ids.get(), (size_t)ntotal * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
	MVS_HIP(hipStreamSynchronize(st));
	ids = std::move(ni);
	idcap = nc;
}
// IndexIDMap::add_with_ids: index->add(n, x); id_map.push_back(ids...)  (src/faiss_extension.cpp:510,607)
void IDMapIndex::add_with_ids(int64_t n, const float *x, const int64_t *xids) {
	use_device();
	if (n <= 0)
		return;
	sub->add(n, x);
	use_device();
	recon_tab.drop();
	grow_ids(ntotal + n, stream);
	const size_t bytes = (size_t)n * sizeof(int64_t);
	// round 6: the ids of DataChunk-sized adds are staged like their rows (FlatIndex::add) -- one H2D copy per full slot, not per call
	if (bytes > PinnedRing::SLOT_BYTES / 2 || (idp_slot >= 0 && idp_bytes + bytes > PinnedRing::SLOT_BYTES))
		flush_ids();
	if (bytes > PinnedRing::SLOT_BYTES / 2) {
		const int slot = id_ring.acquire(bytes);
		memcpy(id_ring.buf[slot], xids, bytes);
		MVS_HIP(hipMemcpyAsync(ids.get() + ntotal, id_ring.buf[slot], bytes, hipMemcpyHostToDevice, stream));
		id_ring.release(slot, stream);
	} else {
		if (idp_slot < 0) {
			idp_slot = id_ring.acquire(PinnedRing::SLOT_BYTES);
			idp_bytes = 0, idp_row0 = ntotal;
		}
		memcpy((char *)id_ring.buf[idp_slot] + idp_bytes, xids, bytes);
		idp_bytes += bytes;
	}
	ntotal = sub->ntotal;
}
void IDMapIndex::flush_ids() {
	if (idp_slot < 0)
		return;
	if (idp_bytes > 0)
		MVS_HIP(hipMemcpyAsync(ids.get() + idp_row0, id_ring.buf[idp_slot], idp_bytes, hipMemcpyHostToDevice, stream));
	id_ring.release(idp_slot, stream);
	idp_slot = -1;
	idp_bytes = 0;
}
void IDMapIndex::add_with_ids_device(int64_t n, const float *d_x, const int64_t *d_ids, hipStream_t st) {
	use_device();
	if (n <= 0)
		return;
	flush_ids();
	stream_wait(st, stream);
	sub->add_device(n, d_x, st);
	recon_tab.drop();
	grow_ids(ntotal + n, st);
	MVS_HIP(hipMemcpyAsync(ids.get() + ntotal, d_ids, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
	stream_wait(stream, st);
	ntotal = sub->ntotal;
}
// IndexIDMap::search: selector tests EXTERNAL ids (IDSelectorTranslated), labels = id_map[internal]
void IDMapIndex::search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I,
                               const mvs_search_params *params, hipStream_t st) {
	use_device();
	flush_ids();
	stream_wait(st, stream); // id_map writes happened on our own stream; the sub-index searches on `st`
	sub->search_mapped(nq, d_x, k, d_D, d_I, params, ids.get(), st);
	kinfo = sub->kinfo;
}
void IDMapIndex::search(int64_t nq, const float *x, int64_t k, float *D, int64_t *I, const mvs_search_params *params) {
	IndexBase::search(nq, x, k, D, I, params);
}
// IndexIDMap::range_search: the wrapped index's hits, the selector on the EXTERNAL ids, labels = id_map[internal]
void IDMapIndex::range_search(int64_t nq, const float *x, float radius, const mvs_search_params *params, RangeResult &out) {
	use_device();
	flush_ids(); // (on our stream, which also carries the queries and the scan)
	const float *d_x = nq > 0 ? stage_queries(nq, x) : nullptr;
	sub->range_search_mapped(nq, d_x, radius, params, ids.get(), out, stream);
	kinfo = sub->kinfo;
}
// IndexIDMap::remove_ids: every row whose EXTERNAL id is a member goes (duplicate external ids are legal: all of them).  The wrapped index
// removes with the mapped selector, the way search_mapped passes the id map, and leaves the marks; the id map compacts with the same scan.
// Over an IVF kind the marks are by stored id and the sub-index renumbers its stored ids (include/mi355_faiss.h "remove_ids": the
// departure from FAISS)
int64_t IDMapIndex::remove_ids(const mvs_search_params *sel, const int64_t *d_idmap, RemoveMarks *) {
	if (d_idmap)
		throw_faiss("mvs::IDMapIndex::remove_ids", __FILE__, "nested IDMap is not supported");
	use_device();
	check_remove_selector(sel);
	flush_ids();
	MVS_HIP(hipStreamSynchronize(stream)); // (the wrapped index reads the id map on its own stream)
	DevBlock<int64_t> ni;
	if (idcap > 0) // (before anything changes: a failure leaves the index as it was)
		ni = DevBlock<int64_t>((size_t)idcap);
	RemoveMarks m;
	const int64_t removed = sub->remove_ids(sel, ids.get(), &m);
	use_device();
	if (removed <= 0)
		return 0;
	launch_remove_compact_i64(ids.get(), m, ni.get(), stream);
	MVS_HIP(hipStreamSynchronize(stream));
	ids = std::move(ni);
	ntotal = sub->ntotal;
	recon_tab.drop();
	return removed;
}
void FlatIndex::range_search(int64_t nq, const float *x, float radius, const mvs_search_params *params, RangeResult &out) {
	use_device();
	range_search_mapped(nq, nq > 0 ? stage_queries(nq, x) : nullptr, radius, params, nullptr, out, stream);
}
bool FlatIndex::named_stat(const char *name, int64_t *v) {
	if (!strcmp(name, "range_rescans")) { // scans repeated because the hit stream was too small, over the index's life
		*v = range_work.rescans;
		return true;
	}
	return false;
}
void IDMapIndex::to_device(int new_device) {
	if (new_device == device)
		return;
	sub->to_device(new_device);
	use_device();
	recon_tab.drop();
	flush_ids();
	MVS_HIP(hipStreamSynchronize(stream));
	id_ring.drop_events();
	if (idcap > 0) {
		MVS_HIP(hipSetDevice(new_device));
		DevBlock<int64_t> ni((size_t)idcap);
		if (ntotal > 0)
			MVS_HIP(hipMemcpyPeer(ni.get(), new_device, ids.get(), device, (size_t)ntotal * sizeof(int64_t)));
		MVS_HIP(hipSetDevice(device)); // (current while the old array is freed)
		ids = std::move(ni);
	}
	move_stream(new_device);
}

IndexBase *IDMapIndex::clone(int on_device) {
	check_device(on_device);
	use_device();
	flush_ids();
	MVS_HIP(hipStreamSynchronize(stream));
	IndexBase *subc = sub->clone(on_device);
	IDMapIndex *c = nullptr;
	try {
		c = new IDMapIndex(subc);
	} catch (...) {
		delete subc;
		throw;
	}
	try {
		c->to_device(on_device); // sub is already there: only moves this wrapper's stream / ids
		c->use_device();
		c->grow_ids(ntotal, c->stream);
		if (ntotal > 0)
			MVS_HIP(hipMemcpyPeer(c->ids.get(), on_device, ids.get(), device, (size_t)ntotal * sizeof(int64_t)));
		c->ntotal = ntotal;
		c->is_idmap2 = is_idmap2;
	} catch (...) {
		delete c;
		throw;
	}
	return c;
}

void FlatIndex::search_mapped(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I,
                              const mvs_search_params *params, const int64_t *d_idmap, hipStream_t st) {
	use_device();
	flush_adds();
	stream_wait(st, stream); // adds were enqueued on our own stream
	search_flat(nq, d_x, k, d_D, d_I, params, d_idmap, st);
}

// ------------------------------------------------------------------------------------------ host images

void FlatIndex::to_host(HostIndex &out) {
	out.kind = MVS_KIND_FLAT;
	out.d = d;
	out.metric = metric;
	out.metric_arg = metric_arg;
	out.ntotal = ntotal;
	out.is_trained = true;
	out.rows.resize((size_t)ntotal * d);
	copy_rows_to_host(out.rows.data());
}
void IDMapIndex::to_host(HostIndex &out) {
	use_device();
	flush_ids();
	MVS_HIP(hipStreamSynchronize(stream));
	refresh_trained();
	out.kind = MVS_KIND_IDMAP;
	out.d = d;
	out.metric = metric;
	out.ntotal = ntotal;
	out.is_trained = is_trained;
	out.sub.reset(new HostIndex);
	sub->to_host(*out.sub);
	out.ids.resize((size_t)ntotal);
	if (ntotal > 0)
		MVS_HIP(hipMemcpy(out.ids.data(), ids.get(), (size_t)ntotal * sizeof(int64_t), hipMemcpyDeviceToHost));
}

IndexBase *index_from_host(const HostIndex &h, int device) {
	CtorDevice scope(device);
	switch (h.kind) {
	case MVS_KIND_FLAT: {
		auto *f = new FlatIndex(h.d, h.metric);
		f->metric_arg = h.metric_arg;
		try {
			if (h.ntotal > 0)
				f->add(h.ntotal, h.rows.data());
		} catch (...) {
			delete f;
			throw;
		}
		return f;
	}
	case MVS_KIND_IDMAP: {
		if (!h.sub)
			throw_faiss("mvs::index_from_host", __FILE__, "IDMap image without a sub-index");
		if (h.sub->ntotal != (int64_t)h.ids.size())
			throw_faiss("faiss::Index* faiss::read_index(...)", "faiss/impl/index_read.cpp",
			            "IDMap id_map size %zu does not match the sub-index ntotal %lld", h.ids.size(),
			            (long long)h.sub->ntotal);
		IndexBase *subi = index_from_host(*h.sub, device);
		IDMapIndex *m = nullptr;
		try {
			m = new IDMapIndex(subi);
		} catch (...) {
			delete subi;
			throw;
		}
		try {
			m->is_idmap2 = h.idmap2;
			m->adopt_ids(h.ids.data(), (int64_t)h.ids.size());
		} catch (...) {
			delete m;
			throw;
		}
		return m;
	}
	case MVS_KIND_IVFFLAT:
		return ivf_from_host(h, device);
	case MVS_KIND_HNSW:
	case MVS_KIND_HNSWSQ:
		return hnsw_from_host(h, device);
	case MVS_KIND_PQ:
		return pq_from_host(h, device);
	case MVS_KIND_IVFPQ:
		return ivfpq_from_host(h, device);
	case MVS_KIND_SQ:
	case MVS_KIND_IVFSQ:
		return sq_from_host(h, device);
	case MVS_KIND_REFINE:
		return refine_from_host(h, device);
	case MVS_KIND_PRETRANSFORM:
		return pretransform_from_host(h, device);
	}
	throw_faiss("mvs::index_from_host", __FILE__, "unknown index kind %d", h.kind);
}

// IndexIDMap image load: the sub-index already holds the rows, only the id_map is missing
void IDMapIndex::adopt_ids(const int64_t *xids, int64_t n) {
	use_device();
	grow_ids(n, stream);
	if (n > 0)
		MVS_HIP(hipMemcpyAsync(ids.get(), xids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, stream));
	MVS_HIP(hipStreamSynchronize(stream));
	ntotal = sub->ntotal;
	is_trained = sub->is_trained;
	recon_tab.drop();
}

// ------------------------------------------------------------------------------------------ factory

// faiss::index_factory subset (faiss/index_factory.cpp) -- the strings the reference and its tests use:
// "Flat" (faiss.test:8), "IDMap,Flat" (faiss2.test:8), "IDMap,IVF1,Flat", "IVF<n>,Flat", "HNSW<M>"; "PQ<M>[x8]" for the glue's IndexPQ branch (:704); "IVF<n>,PQ<M>[x8]", an IndexIVF (:675);
// "SQ8" and "IVF<n>,SQ8" (an IndexIVF too); "<base>,RFlat" / "<base>,Refine(Flat)" over the four quantised kinds (csrc/refine.hip);
// "<t1>,...,<tn>,<sub>" with PCA<o> / PCAW<o> / L2norm in front of any of the above but a refine stage (csrc/pretransform.hip)
static IndexBase *factory_rec(int d, const std::string &desc, int metric, const std::string &full) {
	if (desc.rfind("IDMap2,", 0) == 0 || desc.rfind("IDMap,", 0) == 0) {
		IndexBase *sub = factory_rec(d, desc.substr(desc.find(',') + 1), metric, full);
		try {
			IDMapIndex *m = new IDMapIndex(sub);
			m->is_idmap2 = desc.rfind("IDMap2,", 0) == 0;
			return m;
		} catch (...) {
			delete sub;
			throw;
		}
	}
	if (IndexBase *ix = make_refine_index(d, desc, metric, full)) // (a refine suffix: before the other makers see the string)
		return ix;
	if (desc == "Flat")
		return new FlatIndex(d, metric);
	if (desc.rfind("OPQ", 0) == 0) // a rotation in front of the product quantiser: no such transform on this path
		throw_faiss("faiss::Index* faiss::index_factory(int, const char*, faiss::MetricType)", "faiss/index_factory.cpp",
		            "This index type is not implemented on the MI355X path yet: %s", full.c_str());
	if (IndexBase *ix = make_pretransform_index(d, desc, metric, full, factory_rec)) // "PCA<o>,...", "PCAW<o>,...", "L2norm,...": a chain, then the sub-index by this function
		return ix;
	if (IndexBase *ix = make_ivfpq_index(d, desc, metric)) // (before make_ivf_index, which refuses every IVF string it does not know)
		return ix;
	if (IndexBase *ix = make_sq_index(d, desc, metric)) // ("SQ8" and "IVF<n>,SQ8": also before make_ivf_index)
		return ix;
	if (IndexBase *ix = make_ivf_index(d, desc, metric))
		return ix;
	if (IndexBase *ix = make_hnsw_index(d, desc, metric))
		return ix;
	if (IndexBase *ix = make_pq_index(d, desc, metric))
		return ix;
	throw_faiss("faiss::Index* faiss::index_factory(int, const char*, faiss::MetricType)", "faiss/index_factory.cpp",
	            "could not parse index string %s", full.c_str());
}

IndexBase *index_factory(int d, const char *description, int metric) {
	if (d <= 0)
		throw_faiss("faiss::Index* faiss::index_factory(int, const char*, faiss::MetricType)",
		            "faiss/index_factory.cpp", "invalid dimension %d", d);
	return factory_rec(d, description, metric, description);
}

} // namespace mvs

// =================================================================================================
// C ABI
// =================================================================================================
using namespace mvs;

struct mvs_index {
	IndexBase *impl;
	bool owned;
	mvs_index *sub_handle = nullptr;
	mvs_index *quantizer_handle = nullptr;
	mvs_index *refine_base_handle = nullptr, *refine_store_handle = nullptr;
	mvs_index *pretransform_sub_handle = nullptr;
	SelectorCall selcall; // selector programs: option sel_bitmap_cap_bytes, statistics sel_lowered / sel_admitted of the handle's last call
	std::mutex mu; // the reference's faiss_lock serialises calls per index; be safe for other hosts
};

#define MVS_API_BEGIN                                                                                                  \
	try {
#define MVS_API_END                                                                                                    \
	}                                                                                                                  \
	catch (const std::exception &e) {                                                                                  \
		g_last_error = e.what();                                                                                       \
		return 1;                                                                                                      \
	}                                                                                                                  \
	catch (...) {                                                                                                      \
		g_last_error = "unknown error";                                                                                \
		return 1;                                                                                                      \
	}                                                                                                                  \
	return 0;

extern "C" {

const char *mvs_last_error(void) {
	return g_last_error.c_str();
}
const char *mvs_version(void) {
	return "mi355-faiss 0.1 (drop-in for duckdb-faiss-ext 0.12.1 hot path)";
}
int mvs_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

int mvs_index_factory(mvs_index **out, int d, const char *description, int metric) {
	MVS_API_BEGIN
	*out = nullptr;
	// env MVS_DEVICES=0,1,...,7: the index is created row-sharded / replicated over those devices (csrc/sharded.hip)
	const std::vector<int> devs = shard_devices_from_env();
	IndexBase *impl = devs.size() > 1 ? make_sharded_index(d, description, metric, devs) : index_factory(d, description, metric);
	auto *h = new mvs_index;
	h->impl = impl;
	h->owned = true;
	*out = h;
	MVS_API_END
}
void mvs_index_free(mvs_index *ix) {
	if (!ix)
		return;
	delete ix->sub_handle;
	delete ix->quantizer_handle;
	mvs_index_free(ix->refine_base_handle); // (a borrowed base handle may have lent a quantizer handle itself)
	mvs_index_free(ix->refine_store_handle);
	mvs_index_free(ix->pretransform_sub_handle);
	if (ix->owned) {
		try {
			delete ix->impl;
		} catch (...) {
		}
	}
	delete ix;
}
int mvs_index_d(const mvs_index *ix) {
	return ix->impl->d;
}
int64_t mvs_index_ntotal(const mvs_index *ix) {
	return ix->impl->ntotal;
}
int mvs_index_is_trained(const mvs_index *ix) {
	ix->impl->refresh_trained(); // (wrappers: the wrapped index may have been trained through a borrowed handle)
	return ix->impl->is_trained ? 1 : 0;
}
int mvs_index_metric_type(const mvs_index *ix) {
	return ix->impl->metric;
}
int mvs_index_kind(const mvs_index *ix) {
	return ix->impl->kind;
}
int mvs_index_device(const mvs_index *ix) {
	return ix->impl->device;
}
mvs_index *mvs_index_idmap_sub(mvs_index *ix) {
	if (ix->impl->kind != MVS_KIND_IDMAP)
		return nullptr;
	if (!ix->sub_handle) {
		ix->sub_handle = new mvs_index;
		ix->sub_handle->impl =
		    is_sharded(ix->impl) ? sharded_inner_view(ix->impl) : static_cast<IDMapIndex *>(ix->impl)->sub;
		ix->sub_handle->owned = false;
	}
	return ix->sub_handle;
}
mvs_index *mvs_index_ivf_quantizer(mvs_index *ix) {
	IndexBase *q = ivf_quantizer_of(sharded_inner_view(ix->impl));
	if (!q)
		return nullptr;
	if (!ix->quantizer_handle) {
		ix->quantizer_handle = new mvs_index;
		ix->quantizer_handle->impl = q;
		ix->quantizer_handle->owned = false;
	}
	return ix->quantizer_handle;
}
static mvs_index *borrowed_handle(mvs_index *&slot, IndexBase *impl) {
	if (!impl)
		return nullptr;
	if (!slot) {
		slot = new mvs_index;
		slot->impl = impl;
		slot->owned = false;
	}
	return slot;
}
static IndexBase *unwrap_idmap(IndexBase *p);
mvs_index *mvs_index_refine_base(mvs_index *ix) {
	return borrowed_handle(ix->refine_base_handle, refine_base_of(unwrap_idmap(ix->impl)));
}
mvs_index *mvs_index_refine_store(mvs_index *ix) {
	return borrowed_handle(ix->refine_store_handle, refine_store_of(unwrap_idmap(ix->impl)));
}
int mvs_index_refine_set_k_factor(mvs_index *ix, float k_factor) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	if (!refine_set_k_factor(unwrap_idmap(ix->impl), k_factor))
		throw_faiss("mvs_index_refine_set_k_factor", __FILE__, "not a Refine index");
	MVS_API_END
}
int mvs_index_refine_get_k_factor(mvs_index *ix, float *k_factor) {
	MVS_API_BEGIN
	if (!refine_get_k_factor(unwrap_idmap(ix->impl), k_factor))
		throw_faiss("mvs_index_refine_get_k_factor", __FILE__, "not a Refine index");
	MVS_API_END
}
// ---- pre-transform indexes (csrc/pretransform.hip)
mvs_index *mvs_index_pretransform_sub(mvs_index *ix) {
	return borrowed_handle(ix->pretransform_sub_handle, pretransform_sub_of(unwrap_idmap(ix->impl)));
}
int mvs_index_pretransform_count(const mvs_index *ix) {
	return pretransform_count(unwrap_idmap(ix->impl));
}
int mvs_index_pretransform_info(const mvs_index *ix, int i, int *type, int *d_in, int *d_out, int *have_bias, int *is_trained) {
	MVS_API_BEGIN
	pretransform_info(unwrap_idmap(ix->impl), i, type, d_in, d_out, have_bias, is_trained);
	MVS_API_END
}
int mvs_index_pretransform_get_linear(mvs_index *ix, int i, float *A, float *b) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	pretransform_get_linear(unwrap_idmap(ix->impl), i, A, b);
	MVS_API_END
}
int mvs_index_pretransform_set_linear(mvs_index *ix, int i, const float *A, const float *b) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	pretransform_set_linear(unwrap_idmap(ix->impl), i, A, b);
	ix->impl->refresh_trained();
	MVS_API_END
}
int mvs_index_pretransform_get_pca(mvs_index *ix, int i, float *mean, float *eigenvalues) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	pretransform_get_pca(unwrap_idmap(ix->impl), i, mean, eigenvalues);
	MVS_API_END
}
int mvs_index_pretransform_apply(mvs_index *ix, int64_t n, const float *x, float *out) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	pretransform_apply(unwrap_idmap(ix->impl), n, x, out);
	MVS_API_END
}
int mvs_index_pretransform_apply_device(mvs_index *ix, int64_t n, const float *d_x, float *d_out, void *stream) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	pretransform_apply_device(unwrap_idmap(ix->impl), n, d_x, d_out, (hipStream_t)stream);
	MVS_API_END
}
static IndexBase *unwrap_idmap(IndexBase *p) {
	p = sharded_inner_view(p); // a sharded index answers for its first shard / replica
	while (p->kind == MVS_KIND_IDMAP)
		p = static_cast<IDMapIndex *>(p)->sub;
	return p;
}
int64_t mvs_index_ivf_nlist(const mvs_index *ix) {
	return ivf_nlist_of(unwrap_idmap(ix->impl));
}
int mvs_index_ivf_get_centroids(mvs_index *ix, float *out) {
	MVS_API_BEGIN
	if (!ivf_get_centroids(unwrap_idmap(ix->impl), out))
		throw_faiss("mvs_index_ivf_get_centroids", __FILE__, "not an IVF index");
	MVS_API_END
}
int mvs_index_ivf_set_centroids(mvs_index *ix, const float *centroids) {
	MVS_API_BEGIN
	bool ok = true, trained = true;
	sharded_for_each(ix->impl, [&](IndexBase *top) { // every row shard probes the same lists
		IndexBase *p = top;
		while (p->kind == MVS_KIND_IDMAP)
			p = static_cast<IDMapIndex *>(p)->sub;
		ok = ok && ivf_set_centroids(p, centroids);
		trained = trained && p->is_trained; // (an IVFPQ index also needs its codebooks, an IVF<n>,SQ8 index its range)
		for (IndexBase *w = top; w->kind == MVS_KIND_IDMAP; w = static_cast<IDMapIndex *>(w)->sub)
			w->is_trained = p->is_trained;
	});
	if (!ok)
		throw_faiss("mvs_index_ivf_set_centroids", __FILE__, "not an IVF index");
	ix->impl->is_trained = trained;
	MVS_API_END
}
int mvs_index_hnsw_set_ef_construction(mvs_index *ix, int v) {
	MVS_API_BEGIN
	bool ok = true;
	sharded_for_each(ix->impl, [&](IndexBase *top) { // every replica builds with the same parameter
		IndexBase *p = top;
		while (p->kind == MVS_KIND_IDMAP)
			p = static_cast<IDMapIndex *>(p)->sub;
		ok = ok && hnsw_set_ef_construction(p, v);
	});
	if (!ok)
		throw_faiss("mvs_index_hnsw_set_ef_construction", __FILE__, "not an HNSW index");
	MVS_API_END
}
int mvs_index_hnsw_get_ef_construction(mvs_index *ix) {
	return hnsw_get_ef_construction(unwrap_idmap(ix->impl));
}
int64_t mvs_index_hnsw_graph_info(mvs_index *ix, int *max_level, int *entry_point) {
	try {
		return hnsw_graph_info(unwrap_idmap(ix->impl), max_level, entry_point);
	} catch (...) {
		return -1;
	}
}
int mvs_index_hnsw_walk_stats(mvs_index *ix, double *evaluations, double *f32_rows, double *bf16_rows) {
	MVS_API_BEGIN
	if (!hnsw_walk_stats(unwrap_idmap(ix->impl), evaluations, f32_rows, bf16_rows))
		throw_faiss("mvs_index_hnsw_walk_stats", __FILE__, "not an HNSW index");
	MVS_API_END
}
int mvs_index_hnsw_get_graph(mvs_index *ix, int32_t *levels, int64_t *offsets, int32_t *neighbors) {
	MVS_API_BEGIN
	if (!hnsw_get_graph(unwrap_idmap(ix->impl), levels, offsets, neighbors))
		throw_faiss("mvs_index_hnsw_get_graph", __FILE__, "not an HNSW index");
	MVS_API_END
}

int mvs_index_pq_info(const mvs_index *ix, int *M, int *nbits) {
	MVS_API_BEGIN
	if (!pq_info(unwrap_idmap(ix->impl), M, nbits))
		throw_faiss("mvs_index_pq_info", __FILE__, "not a PQ index");
	MVS_API_END
}
int mvs_index_pq_get_centroids(mvs_index *ix, float *out) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	if (!pq_get_centroids(unwrap_idmap(ix->impl), out))
		throw_faiss("mvs_index_pq_get_centroids", __FILE__, "not a PQ index");
	MVS_API_END
}
int mvs_index_pq_set_centroids(mvs_index *ix, const float *centroids) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	IndexBase *p = unwrap_idmap(ix->impl);
	if (!pq_set_centroids(p, centroids))
		throw_faiss("mvs_index_pq_set_centroids", __FILE__, "not a PQ index");
	for (IndexBase *w = ix->impl; w->kind == MVS_KIND_IDMAP; w = static_cast<IDMapIndex *>(w)->sub)
		w->is_trained = p->is_trained; // (an IVFPQ index also needs its coarse centroids)
	MVS_API_END
}
int mvs_index_pq_get_codes(mvs_index *ix, int64_t row0, int64_t n, uint8_t *out) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	if (!pq_get_codes(unwrap_idmap(ix->impl), row0, n, out))
		throw_faiss("mvs_index_pq_get_codes", __FILE__, "not a PQ index");
	MVS_API_END
}

// the index behind a handle as a coded-lists index of `kind`; the refusal of another kind names the file the kind lives in
static CodedListsIndex *coded_lists_of_kind(const mvs_index *ix, int kind, const char *fn) {
	CodedListsIndex *p = coded_lists_of(unwrap_idmap(ix->impl));
	if (!p || p->kind != kind)
		throw_faiss(fn, kind == MVS_KIND_IVFPQ ? "ivfpq.hip" : "sq.hip", kind == MVS_KIND_IVFPQ ? "not an IVFPQ index" : "not an IVFSQ index");
	return p;
}
static int64_t coded_list_size(const mvs_index *ix, int kind, const char *fn, int64_t list_no) {
	try {
		std::lock_guard<std::mutex> g(const_cast<mvs_index *>(ix)->mu);
		return coded_lists_of_kind(ix, kind, fn)->list_size(list_no);
	} catch (const std::exception &e) {
		g_last_error = e.what();
		return -1;
	}
}
int64_t mvs_index_ivfpq_list_size(const mvs_index *ix, int64_t list_no) {
	return coded_list_size(ix, MVS_KIND_IVFPQ, "mvs_index_ivfpq_list_size", list_no);
}
int mvs_index_ivfpq_get_list(mvs_index *ix, int64_t list_no, int64_t *ids, uint8_t *codes) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	coded_lists_of_kind(ix, MVS_KIND_IVFPQ, "mvs_index_ivfpq_get_list")->get_list(list_no, ids, codes);
	MVS_API_END
}

int mvs_index_sq_get_trained(mvs_index *ix, float *out) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	if (!sq_get_trained(unwrap_idmap(ix->impl), out))
		throw_faiss("mvs_index_sq_get_trained", __FILE__, "not an SQ index");
	MVS_API_END
}
int mvs_index_sq_set_trained(mvs_index *ix, const float *trained) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	IndexBase *p = unwrap_idmap(ix->impl);
	if (!sq_set_trained(p, trained))
		throw_faiss("mvs_index_sq_set_trained", __FILE__, "not an SQ index");
	for (IndexBase *w = ix->impl; w->kind == MVS_KIND_IDMAP; w = static_cast<IDMapIndex *>(w)->sub)
		w->is_trained = p->is_trained; // (an IVF<n>,SQ8 index also needs its coarse centroids)
	MVS_API_END
}
int mvs_index_sq_get_codes(mvs_index *ix, int64_t row0, int64_t n, uint8_t *out) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	if (!sq_get_codes(unwrap_idmap(ix->impl), row0, n, out))
		throw_faiss("mvs_index_sq_get_codes", __FILE__, "not an SQ8 index");
	MVS_API_END
}
int64_t mvs_index_ivfsq_list_size(const mvs_index *ix, int64_t list_no) {
	return coded_list_size(ix, MVS_KIND_IVFSQ, "mvs_index_ivfsq_list_size", list_no);
}
int mvs_index_ivfsq_get_list(mvs_index *ix, int64_t list_no, int64_t *ids, uint8_t *codes) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	coded_lists_of_kind(ix, MVS_KIND_IVFSQ, "mvs_index_ivfsq_get_list")->get_list(list_no, ids, codes);
	MVS_API_END
}

int mvs_index_train(mvs_index *ix, int64_t n, const float *x) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	ix->impl->train(n, x);
	MVS_API_END
}
int mvs_index_add(mvs_index *ix, int64_t n, const float *x) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	ix->impl->add(n, x);
	MVS_API_END
}
int mvs_index_add_with_ids(mvs_index *ix, int64_t n, const float *x, const int64_t *ids) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	ix->impl->add_with_ids(n, x, ids);
	MVS_API_END
}
int mvs_index_search(mvs_index *ix, int64_t n, const float *x, int64_t k, float *distances, int64_t *labels,
                     const mvs_search_params *params) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	SelectorCallScope sc(ix->selcall, params);
	ix->impl->search(n, x, k, distances, labels, params);
	MVS_API_END
}
int mvs_index_range_search(mvs_index *ix, int64_t n, const float *x, float radius, const mvs_search_params *params,
                           mvs_range_result **out) {
	MVS_API_BEGIN
	if (!out)
		throw_faiss("mvs_index_range_search", __FILE__, "null argument");
	*out = nullptr;
	std::lock_guard<std::mutex> g(ix->mu);
	SelectorCallScope sc(ix->selcall, params);
	std::unique_ptr<mvs_range_result> r(new mvs_range_result);
	r->res.clear(n);
	ix->impl->range_search(n, x, radius, params, r->res);
	*out = r.release();
	MVS_API_END
}
int mvs_index_remove_ids(mvs_index *ix, int32_t sel_kind, const void *sel_data, int64_t sel_n, int64_t *n_removed) {
	MVS_API_BEGIN
	if (n_removed)
		*n_removed = 0;
	mvs_search_params p;
	memset(&p, 0, sizeof p);
	p.sel_kind = sel_kind;
	p.sel_data = sel_data;
	p.sel_n = sel_n;
	check_remove_selector(&p);
	std::lock_guard<std::mutex> g(ix->mu);
	SelectorCallScope sc(ix->selcall, &p);
	const int64_t n = ix->impl->remove_ids(&p);
	if (n_removed)
		*n_removed = n;
	MVS_API_END
}
// ---- merge_from and copy_subset_to (csrc/merge.hip): both handles are locked for the call (one lock when they are the same handle)
namespace {
struct TwoLocks {
	std::unique_lock<std::mutex> a, b;
	TwoLocks(const mvs_index *x, const mvs_index *y) {
		if (!x || !y)
			throw_faiss("mvs_index_merge_from", __FILE__, "null argument");
		if (x == y) {
			a = std::unique_lock<std::mutex>(const_cast<mvs_index *>(x)->mu);
			return;
		}
		a = std::unique_lock<std::mutex>(const_cast<mvs_index *>(x)->mu, std::defer_lock);
		b = std::unique_lock<std::mutex>(const_cast<mvs_index *>(y)->mu, std::defer_lock);
		std::lock(a, b);
	}
};
} // namespace
int mvs_index_merge_from(mvs_index *ix, mvs_index *other, int64_t add_id) {
	MVS_API_BEGIN
	TwoLocks g(ix, other);
	ix->impl->merge_from(*other->impl, add_id);
	MVS_API_END
}
int mvs_index_check_compatible_for_merge(const mvs_index *ix, const mvs_index *other) {
	MVS_API_BEGIN
	TwoLocks g(ix, other);
	ix->impl->check_compatible_for_merge(*other->impl);
	MVS_API_END
}
int mvs_index_ivf_copy_subset_to(const mvs_index *ix, mvs_index *other, int subset_type, int64_t a1, int64_t a2) {
	MVS_API_BEGIN
	TwoLocks g(ix, other);
	ix->impl->copy_subset_to(*other->impl, subset_type, a1, a2);
	MVS_API_END
}
// ---- reconstruct (csrc/reconstruct.hip): the entry points are IndexBase's, the same for every kind
int mvs_index_reconstruct(mvs_index *ix, int64_t key, float *recons) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	ix->impl->reconstruct_batch(1, &key, recons);
	MVS_API_END
}
int mvs_index_reconstruct_n(mvs_index *ix, int64_t i0, int64_t ni, float *recons) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	ix->impl->reconstruct_n(i0, ni, recons);
	MVS_API_END
}
int mvs_index_reconstruct_batch(mvs_index *ix, int64_t n, const int64_t *keys, float *recons) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	ix->impl->reconstruct_batch(n, keys, recons);
	MVS_API_END
}
int mvs_index_search_and_reconstruct(mvs_index *ix, int64_t n, const float *x, int64_t k, float *distances, int64_t *labels, float *recons,
                                     const mvs_search_params *params) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	SelectorCallScope sc(ix->selcall, params);
	ix->impl->search_and_reconstruct(n, x, k, distances, labels, recons, params);
	MVS_API_END
}
int mvs_index_reconstruct_batch_device(mvs_index *ix, int64_t n, const int64_t *d_keys, float *d_recons, void *stream) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	ix->impl->reconstruct_batch_device(n, d_keys, d_recons, (hipStream_t)stream);
	MVS_API_END
}
int mvs_index_search_and_reconstruct_device(mvs_index *ix, int64_t n, const float *d_x, int64_t k, float *d_distances, int64_t *d_labels,
                                            float *d_recons, const mvs_search_params *params, void *stream) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	SelectorCallScope sc(ix->selcall, params);
	ix->impl->search_and_reconstruct_device(n, d_x, k, d_distances, d_labels, d_recons, params, (hipStream_t)stream);
	MVS_API_END
}
int64_t mvs_range_result_nq(const mvs_range_result *r) {
	return r ? (int64_t)r->res.lims.size() - 1 : 0;
}
const int64_t *mvs_range_result_lims(const mvs_range_result *r) {
	return r ? r->res.lims.data() : nullptr;
}
const float *mvs_range_result_distances(const mvs_range_result *r) {
	return r ? r->res.distances.data() : nullptr;
}
const int64_t *mvs_range_result_labels(const mvs_range_result *r) {
	return r ? r->res.labels.data() : nullptr;
}
void mvs_range_result_free(mvs_range_result *r) {
	delete r;
}
int mvs_index_to_gpu(mvs_index *ix, int device) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	ix->impl->to_device(device);
	MVS_API_END
}
int mvs_index_clone_to_gpu(mvs_index **out, const mvs_index *src, int device) {
	MVS_API_BEGIN
	*out = nullptr;
	std::lock_guard<std::mutex> g(const_cast<mvs_index *>(src)->mu);
	IndexBase *impl = nullptr;
	if (device < 0) { // faiss_to_gpu(name, -1): every device of MVS_DEVICES, or all visible ones
		std::vector<int> devs = shard_devices_from_env();
		if (devs.empty())
			for (int i = 0; i < mvs_device_count(); ++i)
				devs.push_back(i);
		HostIndex img;
		src->impl->to_host(img);
		impl = shard_from_host(img, devs);
	} else {
		impl = src->impl->clone(device);
	}
	impl->adopt_tuning(src->impl->tune_);
	auto *h = new mvs_index;
	h->impl = impl;
	h->owned = true;
	*out = h;
	MVS_API_END
}
int mvs_index_shard_to_gpus(mvs_index *ix, const int *devices, int ndev) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	if (ndev <= 0 || !devices)
		throw_faiss("mvs_index_shard_to_gpus", __FILE__, "Invalid GPU device list");
	if (ix->sub_handle || ix->quantizer_handle) {
		// borrowed views of the old object graph (IndexIDMap::index, IndexIVF::quantizer) die with it
		delete ix->sub_handle;
		delete ix->quantizer_handle;
		ix->sub_handle = ix->quantizer_handle = nullptr;
	}
	HostIndex img;
	ix->impl->to_host(img);
	IndexBase *sharded = shard_from_host(img, std::vector<int>(devices, devices + ndev));
	sharded->adopt_tuning(ix->impl->tune_);
	if (ix->owned)
		delete ix->impl;
	ix->impl = sharded;
	ix->owned = true;
	MVS_API_END
}
int mvs_index_prefilter_stats(mvs_index *ix, int64_t *queries, int64_t *fallback_queries, float *max_rel_err,
                              float *err_bound) {
	MVS_API_BEGIN
	IndexBase *p = sharded_inner_view(ix->impl);
	while (p->kind == MVS_KIND_IDMAP)
		p = static_cast<IDMapIndex *>(p)->sub;
	if (IndexBase *inner = pretransform_sub_of(p)) // (a pre-transform chain: the searching kernels, and their statistics, are the sub-index's)
		p = inner;
	if (p->kind != MVS_KIND_FLAT) {
		// IVF<n>,Flat counts the same two figures for its filters (csrc/ivf.hip named_stat); it keeps no error figures
		int64_t nq = 0, nf = 0;
		if (!p->named_stat("pf_queries", &nq) || !p->named_stat("pf_fallback_queries", &nf))
			throw_faiss("mvs_index_prefilter_stats", __FILE__, "not a Flat index");
		if (queries)
			*queries = nq;
		if (fallback_queries)
			*fallback_queries = nf;
		if (max_rel_err)
			*max_rel_err = 0.f;
		if (err_bound)
			*err_bound = 0.f;
		return 0;
	}
	auto *f = static_cast<FlatIndex *>(p);
	if (queries)
		*queries = f->pf_queries_total;
	if (fallback_queries)
		*fallback_queries = f->pf_fallback_total;
	if (max_rel_err)
		*max_rel_err = f->pf_max_rel_err;
	if (err_bound)
		*err_bound = prefilter_cerr(f->d);
	MVS_API_END
}
int mvs_index_collect_stats(mvs_index *ix, int64_t *queries, int64_t *candidates, int64_t *overflows) {
	MVS_API_BEGIN
	IndexBase *p = sharded_inner_view(ix->impl);
	while (p->kind == MVS_KIND_IDMAP)
		p = static_cast<IDMapIndex *>(p)->sub;
	if (IndexBase *inner = pretransform_sub_of(p)) // (a pre-transform chain: the searching kernels, and their statistics, are the sub-index's)
		p = inner;
	if (p->kind != MVS_KIND_FLAT) {
		if (p->collect_stats(queries, candidates, overflows)) // IVF: its own coarse filter (csrc/ivf_collect.hip)
			return 0;
		throw_faiss("mvs_index_collect_stats", __FILE__, "not a Flat or IVF index");
	}
	auto *f = static_cast<FlatIndex *>(p);
	if (queries)
		*queries = f->cl_queries_total;
	if (candidates) // (the bucketed finish re-scores the survivors of the final-bound filter only: admitted - (admitted - re-scored) of those searches)
		*candidates = f->cl_candidates_total - (f->cl_admitted_in_fb - f->cl_rescored_total);
	if (overflows)
		*overflows = f->cl_overflows;
	MVS_API_END
}
int mvs_trace_push(const char *name) {
	trace_push(name ? name : "mvs");
	return 0;
}
int mvs_trace_pop(void) {
	trace_pop();
	return 0;
}
int mvs_index_get_stat(mvs_index *ix, const char *name, int64_t *value) {
	MVS_API_BEGIN
	IndexBase *p = sharded_inner_view(ix->impl);
	while (p->kind == MVS_KIND_IDMAP)
		p = static_cast<IDMapIndex *>(p)->sub;
	if (name && strncmp(name, "pretransform_", 13) != 0)
		if (IndexBase *inner = pretransform_sub_of(p)) // (every other statistic of a pre-transform index is its sub-index's)
			p = inner;
	if (!name || !value)
		throw_faiss("mvs_index_get_stat", __FILE__, "null argument");
	if (!strcmp(name, "device_bytes_live")) { // of the process, whatever the handle: device memory held through csrc/dev_mem.h's owners
		*value = g_dev_bytes_live.load();
	} else if (!strcmp(name, "flat_outlier_rows")) { // rows of a Flat index kept out of its coarse-filter store (found so far; csrc/flat_collect.hip)
		if (p->kind != MVS_KIND_FLAT)
			throw_faiss("mvs_index_get_stat", __FILE__, "%s: not a Flat index", name);
		*value = static_cast<FlatIndex *>(p)->outl_total;
	} else if (!strcmp(name, "cl_store_i8")) { // 1: the Flat index's coarse filter runs on the int8 store (csrc/flat_collect.hip "int8 store")
		if (p->kind != MVS_KIND_FLAT)
			throw_faiss("mvs_index_get_stat", __FILE__, "%s: not a Flat index", name);
		const auto *f = static_cast<FlatIndex *>(p);
		*value = f->cl_i8 && f->i8_state == 1 ? 1 : 0;
	} else if (!strcmp(name, "cl_row_classes")) { // row classes per query of the Flat index's last coarse pass (csrc/flat_collect.hip collect_slot_stride)
		if (p->kind != MVS_KIND_FLAT)
			throw_faiss("mvs_index_get_stat", __FILE__, "%s: not a Flat index", name);
		*value = static_cast<FlatIndex *>(p)->cl_row_classes;
	} else if (!strcmp(name, "cl_scan_items") || !strcmp(name, "cl_scan_ranges")) {
		// the plan of the Flat index's last d <= 128 scan launch: row ranges, and items = ranges x query blocks (csrc/flat_collect.h)
		if (p->kind != MVS_KIND_FLAT)
			throw_faiss("mvs_index_get_stat", __FILE__, "%s: not a Flat index", name);
		const auto *f = static_cast<FlatIndex *>(p);
		*value = !strcmp(name, "cl_scan_items") ? f->cl_scan_items : f->cl_scan_ranges;
	} else if (!strcmp(name, "coarse_bf16_queries") || !strcmp(name, "coarse_bf16_exhaustive") || !strcmp(name, "coarse_bf16_candidates")) {
		// IVF: queries whose coarse quantisation ran on csrc/coarse_bf16.hip / of those, computed against every centroid
		IndexBase *qz = ivf_quantizer_of(p);
		if (!qz || qz->kind != MVS_KIND_FLAT)
			throw_faiss("mvs_index_get_stat", __FILE__, "%s: not an IVF index with a Flat quantizer", name);
		auto *f = static_cast<FlatIndex *>(qz);
		if (!strcmp(name, "coarse_bf16_queries")) {
			*value = f->cb16_queries;
		} else if (!strcmp(name, "coarse_bf16_candidates")) { // candidates re-scored exactly in the LAST call (its last piece), summed
			int64_t sum = 0;
			if (f->ws_cb16.p && f->cb16_last_nq > 0) {
				f->use_device();
				MVS_HIP(hipDeviceSynchronize());
				std::vector<int> cc((size_t)f->cb16_last_nq);
				MVS_HIP(hipMemcpy(cc.data(), (const char *)f->ws_cb16.p + f->cb16_ccount_off, cc.size() * sizeof(int), hipMemcpyDeviceToHost));
				for (int v : cc)
					sum += v > 0 ? v : 0;
			}
			*value = sum;
		} else {
			unsigned long long v = 0;
			if (f->ws_cb16.p) {
				f->use_device();
				MVS_HIP(hipDeviceSynchronize());
				MVS_HIP(hipMemcpy(&v, (const char *)f->ws_cb16.p + f->cb16_stats_off, sizeof v, hipMemcpyDeviceToHost));
			}
			*value = (int64_t)v;
		}
	} else if (!strcmp(name, "sel_lowered")) { // the handle's last call with a selector program: 0 not lowered | 1 bitmap | 2 batch (csrc/selector_lower.hip)
		*value = ix->selcall.lowered;
	} else if (!strcmp(name, "sel_admitted")) { // ... and the admitted ids it counted
		*value = ix->selcall.admitted;
	} else if (!strcmp(name, "recon_pq_lds")) {
		// the handle's last reconstruction that decoded PQ codes: 1 codebooks in LDS, 0 through L2, -1 none yet (csrc/reconstruct.hip)
		*value = ix->impl->recon_last_pq_lds;
	} else if (!p->named_stat(name, value)) {
		throw_faiss("mvs_index_get_stat", __FILE__, "unknown statistic %s", name);
	}
	MVS_API_END
}
int mvs_index_shadow_stats(mvs_index *ix, int64_t *stats /* [8] */, double *build_seconds) {
	MVS_API_BEGIN
	IndexBase *p = sharded_inner_view(ix->impl);
	while (p->kind == MVS_KIND_IDMAP)
		p = static_cast<IDMapIndex *>(p)->sub;
	if (IndexBase *inner = pretransform_sub_of(p)) // (a pre-transform chain: the searching kernels, and their statistics, are the sub-index's)
		p = inner;
	if (p->kind != MVS_KIND_FLAT)
		throw_faiss("mvs_index_shadow_stats", __FILE__, "not a Flat index");
	auto *f = static_cast<FlatIndex *>(p);
	if (stats) {
		stats[0] = f->shadow_state, stats[1] = f->shadow ? f->shadow_rows : -1, stats[2] = f->shadow_queries, stats[3] = f->shadow_unproven;
		stats[4] = f->shadow_builds, stats[5] = f->shadow_extends, stats[6] = f->shadow ? (int64_t)f->shadow->device_bytes() : 0;
		stats[7] = f->shadow ? ivf_nlist_of(f->shadow) : 0;
	}
	if (build_seconds)
		*build_seconds = f->shadow_build_seconds;
	MVS_API_END
}
int mvs_index_ivf_probe_stats(mvs_index *ix, int64_t *pairs, int64_t *pairs_scanned, int64_t *forced_drains, int64_t *admitted) {
	MVS_API_BEGIN
	IndexBase *p = sharded_inner_view(ix->impl);
	while (p->kind == MVS_KIND_IDMAP)
		p = static_cast<IDMapIndex *>(p)->sub;
	if (IndexBase *inner = pretransform_sub_of(p)) // (a pre-transform chain: the searching kernels, and their statistics, are the sub-index's)
		p = inner;
	if (p->kind == MVS_KIND_FLAT && static_cast<FlatIndex *>(p)->shadow) // a Flat index answering through its shadow clustering
		p = static_cast<FlatIndex *>(p)->shadow;
	if (!p->probe_stats(pairs, pairs_scanned, forced_drains, admitted)) {
		if (p->kind != MVS_KIND_FLAT)
			throw_faiss("mvs_index_ivf_probe_stats", __FILE__, "not an IVF index");
		// a Flat index: no probes; `admitted` = candidates its coarse filter admitted in the last search (mvs_index_collect_stats counts
		// the re-scored ones)
		if (pairs)
			*pairs = 0;
		if (pairs_scanned)
			*pairs_scanned = 0;
		if (forced_drains)
			*forced_drains = 0;
		if (admitted)
			*admitted = static_cast<FlatIndex *>(p)->cl_last_candidates;
	}
	MVS_API_END
}
int mvs_index_shard_info(const mvs_index *ix, int *devices, int max_devices, int64_t *rows_per_shard,
                         int64_t *last_tie_queries) {
	return sharded_info(ix->impl, devices, max_devices, rows_per_shard, last_tie_queries);
}
int mvs_index_add_device(mvs_index *ix, int64_t n, const float *d_x, const int64_t *d_ids, void *stream) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	if (d_ids)
		ix->impl->add_with_ids_device(n, d_x, d_ids, (hipStream_t)stream);
	else
		ix->impl->add_device(n, d_x, (hipStream_t)stream);
	MVS_API_END
}
int mvs_index_search_device(mvs_index *ix, int64_t n, const float *d_x, int64_t k, float *d_distances,
                            int64_t *d_labels, const mvs_search_params *params, void *stream) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	if (k <= 0)
		throw_faiss("virtual void faiss::Index::search(...) const", "faiss/Index.cpp", "Error: 'k > 0' failed");
	SelectorCallScope sc(ix->selcall, params);
	ix->impl->search_device(n, d_x, k, d_distances, d_labels, params, (hipStream_t)stream);
	MVS_API_END
}
int mvs_index_set_label_offset(mvs_index *ix, int64_t offset) {
	MVS_API_BEGIN
	ix->impl->set_label_offset(offset);
	MVS_API_END
}

int mvs_write_index(const mvs_index *ix, const char *filename) {
	MVS_API_BEGIN
	write_index_file(ix->impl, filename);
	MVS_API_END
}
int mvs_read_index(mvs_index **out, const char *filename) {
	MVS_API_BEGIN
	*out = nullptr;
	IndexBase *impl = read_index_file(filename);
	auto *h = new mvs_index;
	h->impl = impl;
	h->owned = true;
	*out = h;
	MVS_API_END
}

int mvs_merge_shards(int metric, int64_t n, int64_t k, int nshard, const float *D, const int64_t *I, float *D_out,
                     int64_t *I_out) {
	MVS_API_BEGIN
	merge_shards_host(metric, n, k, nshard, D, I, D_out, I_out);
	MVS_API_END
}

int mvs_merge_records_device(int metric, int64_t n, int kk, int kout, int nshard, const int64_t *d_records, int raw,
                             float *d_D_out, int64_t *d_I_out, void *stream) {
	MVS_API_BEGIN
	launch_merge_records(metric, d_records, nshard, n, kk, kout, raw != 0, d_D_out, d_I_out, (hipStream_t)stream);
	MVS_API_END
}

int mvs_merge_shards_raw(int metric, int64_t n, int64_t kk, int nshard, const float *D, const int64_t *I, float *D_out,
                         int64_t *I_out) {
	MVS_API_BEGIN
	merge_shards_raw_host(metric, n, kk, nshard, D, I, D_out, I_out);
	MVS_API_END
}
int mvs_finish_ip_ties(int64_t n, int64_t k, int64_t kk, const float *raw_D, const int64_t *raw_I, int64_t nf,
                       const int64_t *flagged, const int64_t *first_rows, float *D_out, int64_t *I_out) {
	MVS_API_BEGIN
	finish_ip_ties_host(n, k, kk, raw_D, raw_I, nf, flagged, first_rows, D_out, I_out);
	MVS_API_END
}
int mvs_index_tie_candidates_device(mvs_index *ix, int64_t nf, const float *d_xf, const float *d_T, int64_t k,
                                    int64_t *d_rows_out, const mvs_search_params *params, void *stream) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	if (ix->impl->kind != MVS_KIND_FLAT || is_sharded(ix->impl))
		throw_faiss("mvs_index_tie_candidates_device", __FILE__, "a plain single-device Flat index is required");
	auto *f = static_cast<FlatIndex *>(ix->impl);
	hipStream_t st = (hipStream_t)stream;
	f->use_device();
	stream_wait(st, f->stream);
	SelectorCallScope sc(ix->selcall, params);
	SelectorDev sel = f->upload_selector(params, nullptr, st);
	f->tie_candidates(nf, d_xf, d_T, k, d_rows_out, sel, nullptr, st);
	f->offset_rows(d_rows_out, nf * k, st); // shard rows -> global rows (label offset)
	MVS_API_END
}
int mvs_index_ivf_tie_emit_device(mvs_index *ix, int64_t nf, const int *d_flag, const float *d_x, const float *d_T, int64_t k,
                                  float *d_v_out, int64_t *d_id_out, int *d_rank_out, const mvs_search_params *params,
                                  void *stream) {
	MVS_API_BEGIN
	std::lock_guard<std::mutex> g(ix->mu);
	if (ix->impl->kind != MVS_KIND_IVFFLAT || is_sharded(ix->impl))
		throw_faiss("mvs_index_ivf_tie_emit_device", __FILE__, "a plain single-device IVF index is required");
	// (the coarse assignment the call reuses belongs to ONE batch -- another pointer is another batch as far as anyone can tell)
	if (nf > 0 && ix->impl->last_batch_ptr() != d_x)
		throw_faiss("mvs_index_ivf_tie_emit_device", __FILE__, "the batch at %p is not the one of the search that has just run on this index (%p)",
		            (const void *)d_x, (const void *)ix->impl->last_batch_ptr());
	if (nf > 0)
		ix->impl->tie_emit(d_flag, (int)nf, d_x, d_T, k, params, nullptr, d_v_out, d_id_out, d_rank_out, (hipStream_t)stream);
	MVS_API_END
}
int mvs_synth_uniform_device(float *d_out, int64_t n_rows, int d, uint64_t seed, int64_t row0, void *stream) {
	MVS_API_BEGIN
	launch_synth_uniform(d_out, n_rows, d, seed, row0, (hipStream_t)stream);
	MVS_API_END
}
int mvs_synth_clustered_device(float *d_out, int64_t n_rows, int d, uint64_t seed, int64_t row0, int n_centers,
                               float sigma, void *stream) {
	MVS_API_BEGIN
	launch_synth_clustered(d_out, n_rows, d, seed, row0, n_centers, sigma, (hipStream_t)stream);
	MVS_API_END
}

int mvs_debug_mfma_bf16_16x16x32(const uint16_t *A, const uint16_t *Bt, const float *C, float *D, int64_t ntiles) {
	MVS_API_BEGIN
	if (ntiles <= 0)
		return 0;
	DevBuf a, b, c, d;
	a.reserve((size_t)ntiles * 512 * 2), b.reserve((size_t)ntiles * 512 * 2), c.reserve((size_t)ntiles * 256 * 4), d.reserve((size_t)ntiles * 256 * 4);
	MVS_HIP(hipMemcpy(a.p, A, (size_t)ntiles * 512 * 2, hipMemcpyHostToDevice));
	MVS_HIP(hipMemcpy(b.p, Bt, (size_t)ntiles * 512 * 2, hipMemcpyHostToDevice));
	MVS_HIP(hipMemcpy(c.p, C, (size_t)ntiles * 256 * 4, hipMemcpyHostToDevice));
	launch_mfma_bf16_probe((const unsigned short *)a.p, (const unsigned short *)b.p, (const float *)c.p, (float *)d.p, ntiles, nullptr);
	MVS_HIP(hipDeviceSynchronize());
	MVS_HIP(hipMemcpy(D, d.p, (size_t)ntiles * 256 * 4, hipMemcpyDeviceToHost));
	MVS_API_END
}
int mvs_index_last_kernel_info(const mvs_index *ix, mvs_kernel_info *out) {
	MVS_API_BEGIN
	*out = ix->impl->kinfo;
	MVS_API_END
}
int mvs_index_set_kernel_timing(mvs_index *ix, int enabled) {
	MVS_API_BEGIN
	ix->impl->set_timing(enabled != 0);
	MVS_API_END
}
int mvs_index_kernel_time_stats(mvs_index *ix, int *count, double *total_ms) {
	MVS_API_BEGIN
	ix->impl->resolve_timing(count, total_ms);
	MVS_API_END
}
int mvs_index_set_option(mvs_index *ix, const char *key, int64_t value) {
	MVS_API_BEGIN
	if (key && !strcmp(key, "sel_bitmap_cap_bytes")) { // (of the handle, whatever its kind: include/mi355_faiss.h "selector programs")
		if (value < 0)
			throw_faiss("mvs_index_set_option", __FILE__, "sel_bitmap_cap_bytes = %lld: 0 (automatic) or a number of bytes", (long long)value);
		ix->selcall.cap_bytes = value;
		return 0;
	}
	if (!ix->impl->set_option(key, value))
		throw_faiss("mvs_index_set_option", __FILE__, "unknown option %s", key);
	MVS_API_END
}

} // extern "C"

namespace mvs {
namespace {
struct Roctx {
	int (*push)(const char *) = nullptr;
	int (*pop)() = nullptr;
	Roctx() {
		bool want = false;
		if (const char *e = getenv("MVS_ROCTX"))
			want = e[0] && e[0] != '0';
		for (const char *v : {"ROCP_TOOL_LIBRARIES", "ROCPROFILER_REGISTER_LIBRARY", "HSA_TOOLS_LIB", "LD_PRELOAD"})
			if (const char *e = getenv(v))
				want = want || strstr(e, "rocprof") != nullptr;
		if (!want)
			return;
		for (const char *n : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "/opt/rocm/lib/librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
			void *h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
			if (!h)
				continue;
			push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
			pop = (int (*)())dlsym(h, "roctxRangePop");
			if (push && pop)
				return;
			push = nullptr, pop = nullptr;
		}
	}
};
const Roctx &roctx() {
	static const Roctx r;
	return r;
}
} // namespace
void trace_push(const char *name) {
	const Roctx &r = roctx();
	if (r.push)
		(void)r.push(name);
}
void trace_pop() {
	const Roctx &r = roctx();
	if (r.pop)
		(void)r.pop();
}
// Per-index tuning (round 5).  Every knob below used to be a process-wide int set through whichever index
// happened to receive set_option -- DuckDB searches different indexes from different threads, so one index's A/B switch changed
// the path (and raced with the launches) of another.  Now an index owns its Tuning; use_device(), the first statement of every
// entry point, makes it the calling thread's current one; the launch functions read tune().x.
static thread_local const Tuning *t_tune = nullptr;
const Tuning &tune() {
	static const Tuning defaults;
	return t_tune ? *t_tune : defaults;
}
void set_current_tuning(const Tuning *t) {
	t_tune = t;
}
void forget_current_tuning(const Tuning *t) {
	if (t_tune == t)
		t_tune = nullptr;
}
bool IndexBase::set_tuning(const char *key, int64_t v) {
	struct Key {
		const char *name;
		int Tuning::*field;
		bool flag; // v != 0 (else the value)
	};
	static const Key keys[] = {
	    {"ivf_coarse_mfma", &Tuning::coarse_mfma, false},  // IVF coarse distance matrix on the f32 matrix pipe (1) or the vector ALU (0); same bits
	    {"ivf_cl_xcd", &Tuning::ivf_cl_xcd, false},        // IVF coarse filter: items of one list on one XCD (1) or dealt round-robin over the XCDs (0)
	    {"ivf_coarse_select", &Tuning::coarse_select, true}, // IVF coarse quantiser: distance matrix + selection (1) or the k-list kernels (0)
	    {"ivf_coarse_bf16", &Tuning::coarse_bf16, true},     // L2 coarse quantiser: bf16 filter + exact re-scoring (1, csrc/coarse_bf16.hip) or distance matrix + selection (0)
	    {"cl_bound_mode", &Tuning::cl_bound_mode, false},  // bf16 rounding term of the coarse filter's bound: actual residual norms (1) | worst case (0)
	    {"cl_tab", &Tuning::cl_tab, true},                // d <= 128 scan: pass bounds through the global table (1, default) or derived per wave (0: round 3)
	    {"mfma_global_lists", &Tuning::mfma_global_lists, false},
	    {"mfma_nsplit", &Tuning::mfma_nsplit, false},
	};
	for (const Key &e : keys) {
		if (strcmp(key, e.name))
			continue;
		tune_.*(e.field) = e.flag ? v != 0 : (int)v;
		return true;
	}
	return false;
}
bool FlatIndex::set_option(const char *key, int64_t v) {
	if (set_tuning(key, v))
		return true;
	if (!strcmp(key, "cl_i8")) { // d <= 128 coarse filter: the int8 store where it is chosen (1, default) or always the bf16 store (0)
		cl_i8 = v != 0;
		return true;
	}
	if (!strcmp(key, "cl_classes")) { // tests: 16 | 32 = the int8 store's row classes for k <= 16; 0 = the rule (stat cl_row_classes)
		if (v != 0 && v != 16 && v != 32)
			throw_faiss("set_option", __FILE__, "cl_classes: 0, 16 or 32");
		cl_classes = (int)v;
		return true;
	}
	if (!strcmp(key, "outlier_rows")) { // 0: no row is kept out of the coarse-filter store (round 5; takes effect at the store's next first build)
		outlier_rows = v != 0;
		return true;
	}
	if (!strcmp(key, "lazy_adds")) { // 0: every add() reaches the device at once (round 5's ingest, for A/B)
		flush_adds();
		lazy_adds = v != 0;
		return true;
	}
	if (!strcmp(key, "metric_arg_bits")) { // faiss::Index::metric_arg as IEEE-754 bits (the option channel carries integers)
		const uint32_t b = (uint32_t)v;
		memcpy(&metric_arg, &b, 4);
		return true;
	}
	if (!strcmp(key, "force_staged")) { // per-pair path on the LDS-staged flat_direct kernel instead of the scan kernel
		force_staged = v != 0;
		return true;
	}
	if (!strcmp(key, "prefilter")) { // -1 auto, 0 off (exact f32 kernel only), 1 wherever the bf16x3 kernel supports the shape
		prefilter_mode = (int)v;
		return true;
	}
	if (!strcmp(key, "tie_from_candidates")) {
		tie_from_candidates = v != 0;
		return true;
	}
	if (!strcmp(key, "cl_k32")) {
		cl_k32 = v != 0;
		return true;
	}
	if (!strcmp(key, "flat_shadow")) { // -1 auto (built when the coarse filter admits thousands of rows per query), 0 never, 1 at once
		shadow_mode = (int)v;
		if (v != 0 && shadow_state < 0)
			shadow_state = 0;
		return true;
	}
	if (!strcmp(key, "flat_shadow_nprobe")) {
		shadow_nprobe = (int)std::max<int64_t>(1, v);
		return true;
	}
	if (!strcmp(key, "cl_fbucket")) { // 0: the sorted pipeline behind the d = 128 L2 coarse filter (round 4); 1: the bucketed finish
		cl_fbucket = v != 0;
		cl_fbucket_off = false;
		return true;
	}
	if (!strcmp(key, "cl_fpitch")) { // bucket entries per query of the bucketed finish (tests: provokes the overflow)
		cl_fpitch = (int)std::max<int64_t>(64, std::min<int64_t>(16384, (v + 63) / 64 * 64));
		cl_fbucket_off = false;
		return true;
	}
	if (!strcmp(key, "cl_bigk")) { // 0: lists beyond 128 entries on the exact kernels (round 5; A/B)
		cl_bigk = v != 0;
		return true;
	}
	if (!strcmp(key, "cl_est")) { // tests: pretend the previous search had v candidates per query (a sort sized too small is re-run)
		cl_est_per_query = (double)v + 1e-6;
		return true;
	}
	if (!strcmp(key, "cl_defer_count")) { // 1 (default): no host round trip for the candidate count between scan and re-scoring
		cl_defer = v != 0;
		return true;
	}
	if (!strcmp(key, "cl_stream_cap")) { // coarse filter: candidate-stream entries per query (diagnostics: provoke the overflow paths)
		cl_stream_cap_per_query = (int)v;
		return true;
	}
	if (!strcmp(key, "raw_rows")) {
		raw_rows = v != 0;
		return true;
	}
	if (!strcmp(key, "ip_exact_ties")) { // 0: pure (score desc, id asc) order, no tie pass (diagnostics)
		ip_exact_ties = v != 0;
		return true;
	}
	if (!strcmp(key, "force_direct")) {
		force_direct = v != 0;
		return true;
	}
	if (!strcmp(key, "range_stream_cap")) { // range search: entries of the first attempt's hit stream (0: automatic; tests force the rerun)
		range_work.stream_cap = std::max<int64_t>(0, v);
		return true;
	}
	if (!strcmp(key, "range_mfma")) { // range search, BLAS-branch batches: the f32 MFMA kernel (1, default) or the VALU formula mode (0); same bits
		range_use_mfma = v != 0;
		return true;
	}
	return false;
}
} // namespace mvs
