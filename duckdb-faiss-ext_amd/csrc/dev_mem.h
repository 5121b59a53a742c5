// csrc/dev_mem.h -- who owns device memory: one allocation (DevMem, which can regrow and keep a prefix), a grow-only scratch buffer
// (DevBuf), a typed block of fixed size (DevBlock), an array that keeps its contents as it grows (DevKeep) and a derived row store
// (DevRowStore); and who owns pinned host memory (PinnedMem).  Every owner is move-only and frees itself; nothing else in csrc/ allocates
// or frees device memory, and only PinnedRing (csrc/index.hip) pins host memory besides.  Plain C++: the device is reached through
// dev_alloc / dev_free (and dev_zero / dev_copy / dev_sync, which own nothing) and pinned memory through pinned_alloc / pinned_free, so a
// program of its own can compile this header against the host heap (MVS_DEV_MEM_HOST; tests/test_dev_mem_cpu.py), as csrc/flat_collect.h
// under MVS_COLLECT_PLAN_ONLY.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

#ifdef MVS_DEV_MEM_HOST
#include <cstdlib>
#include <cstring>
#include <new>
#else
#include "common.h"
#endif

namespace mvs {

// bytes held through dev_alloc and not yet given back, over the process (statistic device_bytes_live of mvs_index_get_stat)
inline std::atomic<int64_t> g_dev_bytes_live {0};

#ifdef MVS_DEV_MEM_HOST
using dev_stream_t = void *;
inline int g_dev_alloc_fail_at = 0; // test hook: the n-th allocation from now on fails (0: none)
inline void *dev_alloc(size_t bytes) {
	if (g_dev_alloc_fail_at > 0 && --g_dev_alloc_fail_at == 0)
		throw std::bad_alloc();
	void *p = calloc(bytes ? bytes : 1, 1);
	if (!p)
		throw std::bad_alloc();
	g_dev_bytes_live += (int64_t)bytes;
	return p;
}
inline void dev_free(void *p, size_t bytes) {
	free(p);
	g_dev_bytes_live -= (int64_t)bytes;
}
inline void dev_zero(void *p, size_t bytes, dev_stream_t) {
	memset(p, 0, bytes);
}
inline void dev_copy(void *dst, const void *src, size_t bytes, dev_stream_t) {
	memcpy(dst, src, bytes);
}
inline void dev_sync(dev_stream_t) {
}
inline void *pinned_alloc(size_t bytes, bool) {
	void *p = malloc(bytes ? bytes : 1);
	if (!p)
		throw std::bad_alloc();
	return p;
}
inline void pinned_free(void *p) {
	free(p);
}
#else
using dev_stream_t = hipStream_t;
inline void *dev_alloc(size_t bytes) { // on the current device
	void *p = nullptr;
	MVS_HIP(hipMalloc(&p, bytes));
	g_dev_bytes_live += (int64_t)bytes;
	return p;
}
inline void dev_free(void *p, size_t bytes) { // (hipFree waits for the whole device: see FlatIndex::grow for what that costs an ingest)
	(void)hipFree(p);
	g_dev_bytes_live -= (int64_t)bytes;
}
inline void dev_zero(void *p, size_t bytes, dev_stream_t st) {
	MVS_HIP(hipMemsetAsync(p, 0, bytes, st));
}
inline void dev_copy(void *dst, const void *src, size_t bytes, dev_stream_t st) {
	MVS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
}
inline void dev_sync(dev_stream_t st) {
	MVS_HIP(hipStreamSynchronize(st));
}
inline void *pinned_alloc(size_t bytes, bool portable) { // portable: every device of the node may DMA from / into it
	void *p = nullptr;
	MVS_HIP(hipHostMalloc(&p, bytes, portable ? hipHostMallocPortable : hipHostMallocDefault));
	return p;
}
inline void pinned_free(void *p) {
	(void)hipHostFree(p);
}
#endif

// How far a store that keeps its contents grows: from `cap` (0: none yet) to the first step of the rule that holds `need`, in the caller's
// units (rows, bytes or elements)
template <class N>
inline N grown_cap(N cap, N need) {
	N nc = cap ? cap : 4096;
	while (nc < need)
		nc = nc + nc / 2 + 4096;
	return nc;
}

struct DevMem { // one allocation of `cap` bytes, or none
	void *p = nullptr;
	size_t cap = 0;
	DevMem() = default;
	explicit DevMem(size_t bytes) : p(dev_alloc(bytes)), cap(bytes) {
	}
	DevMem(const DevMem &) = delete;
	DevMem &operator=(const DevMem &) = delete;
	DevMem(DevMem &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {
	}
	DevMem &operator=(DevMem &&o) noexcept {
		if (this != &o) {
			release();
			p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0);
		}
		return *this;
	}
	~DevMem() {
		release();
	}
	void release() {
		if (p)
			dev_free(p, cap);
		p = nullptr, cap = 0;
	}
	// room for new_bytes (no-op when they are there), the first keep_bytes kept; with `zero`, every other byte is zero.  The new allocation
	// is made before the old one is touched: a failure leaves this one as it was, and whatever throws later frees the new one.  The stream
	// is synchronised BEFORE the old allocation is freed (as DevRowStore::grow)
	void regrow(size_t new_bytes, size_t keep_bytes, bool zero, dev_stream_t st) {
		if (new_bytes <= cap)
			return;
		DevMem nm(new_bytes);
		if (zero)
			dev_zero(nm.p, new_bytes, st);
		if (keep_bytes > 0 && p)
			dev_copy(nm.p, p, keep_bytes, st);
		dev_sync(st);
		*this = std::move(nm);
	}
};

struct DevBuf : DevMem { // grow-only device scratch (contents NOT preserved on growth)
	void reserve(size_t bytes) {
		if (bytes <= cap)
			return;
		release();
		static_cast<DevMem &>(*this) = DevMem(bytes + bytes / 4 + 256);
	}
};

template <class T>
struct DevBlock : DevMem { // `count` elements of T, exactly; a new block replaces the old one only once it is allocated
	DevBlock() = default;
	explicit DevBlock(size_t count) : DevMem(count * sizeof(T)) {
	}
	T *get() const {
		return (T *)p;
	}
	explicit operator bool() const {
		return p != nullptr;
	}
};

template <class T>
struct DevKeep : DevMem { // array of T that keeps its first `used` elements when it grows, by the stores' rule (grown_cap) in elements
	T *get() const {
		return (T *)p;
	}
	size_t count() const {
		return cap / sizeof(T);
	}
	void ensure(size_t need, size_t used, dev_stream_t st, bool zero = false) {
		if (need > count())
			regrow(grown_cap(count(), need) * sizeof(T), used * sizeof(T), zero, st);
	}
};

struct PinnedMem { // pinned host memory, grow-only (contents NOT preserved on growth)
	void *p = nullptr;
	size_t cap = 0;
	PinnedMem() = default;
	PinnedMem(const PinnedMem &) = delete;
	PinnedMem &operator=(const PinnedMem &) = delete;
	PinnedMem(PinnedMem &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {
	}
	PinnedMem &operator=(PinnedMem &&o) noexcept {
		if (this != &o) {
			release();
			p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0);
		}
		return *this;
	}
	~PinnedMem() {
		release();
	}
	void *reserve(size_t bytes, bool portable = false) {
		if (bytes > cap) {
			release();
			p = pinned_alloc(bytes + bytes / 4 + 256, portable);
			cap = bytes + bytes / 4 + 256;
		}
		return p;
	}
	void release() {
		if (p)
			pinned_free(p);
		p = nullptr, cap = 0;
	}
};

// A row store derived from an index's rows: `cap + pad` rows of row_bytes each and, with side_bytes > 0, as many side values (one per
// row); rows [0, n) are converted, every other byte is zero (the pad rows are what the scans prefetch past the end without clamping)
struct DevRowStore {
	DevMem rows, side;
	size_t row_bytes = 0, side_bytes = 0;
	int64_t pad = 0, cap = 0, n = 0;
	DevRowStore() = default;
	DevRowStore(size_t row_bytes_, size_t side_bytes_, int64_t pad_) : row_bytes(row_bytes_), side_bytes(side_bytes_), pad(pad_) {
	}
	DevRowStore(DevRowStore &&o) noexcept
	    : rows(std::move(o.rows)), side(std::move(o.side)), row_bytes(o.row_bytes), side_bytes(o.side_bytes), pad(o.pad), cap(std::exchange(o.cap, 0)),
	      n(std::exchange(o.n, 0)) {
	}
	DevRowStore &operator=(DevRowStore &&o) noexcept { // (the shape comes along; the source keeps its own and is empty)
		if (this != &o) {
			rows = std::move(o.rows), side = std::move(o.side);
			row_bytes = o.row_bytes, side_bytes = o.side_bytes, pad = o.pad;
			cap = std::exchange(o.cap, 0), n = std::exchange(o.n, 0);
		}
		return *this;
	}
	// room for `nrows` rows, the converted ones kept.  Both arrays are allocated before the old ones are touched: a failure leaves the
	// store as it was.  The stream is synchronised BEFORE the old pair is freed -- dev_free waits for the device, the copy must not be
	// what it waits for with the old arrays already gone
	void grow(int64_t nrows, dev_stream_t st) {
		if (nrows <= cap && rows.p)
			return;
		const size_t total = (size_t)(nrows + pad);
		DevMem nr(total * row_bytes), ns;
		if (side_bytes)
			ns = DevMem(total * side_bytes);
		dev_zero(nr.p, nr.cap, st);
		if (side_bytes)
			dev_zero(ns.p, ns.cap, st);
		if (n > 0) {
			dev_copy(nr.p, rows.p, (size_t)n * row_bytes, st);
			if (side_bytes)
				dev_copy(ns.p, side.p, (size_t)n * side_bytes, st);
		}
		dev_sync(st);
		rows = std::move(nr), side = std::move(ns);
		cap = nrows;
	}
	void drop() {
		rows.release(), side.release();
		cap = n = 0;
	}
};

} // namespace mvs
