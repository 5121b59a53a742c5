// csrc/binary.hip -- binary indexes: "BFlat" (faiss::IndexBinaryFlat) and "IDMap,BFlat" / "IDMap2,BFlat" (faiss::IndexBinaryIDMap over it).
// Bit vectors of d bits, compared by Hamming distance, exact by construction.  The contract is the "binary indexes" section of
// include/mi355_faiss.h; the design, the selection rule and the measured table are DESIGN.md 3.15.
//
// Store.  Two copies of the rows: `codes` [cap][code_size] bytes as they arrive (reconstruct, write_index) and `tiled`, word-major tiles of
// 64 rows: word w of row 64 t + l is tiled[(t wpr + w) 64 + l], wpr = ceil(d / 32), the last word padded with zero bits.  One wave loads
// word w of a tile's 64 rows as ONE coalesced 256-byte access; binary_pack_kernel builds the tiles of the rows an add brought.
//
// Scan (binary_scan_kernel).  A wave owns a tile: lane l holds the wpr words of row 64 t + l in VGPRs.  The queries of the block arrive as
// wave-uniform operands (scalar loads of the packed query words), so a pair costs v_xor_b32 + v_bcnt_u32_b32 per 32 bits and ONE compare.
// No k-lists in the scan: a row is admitted iff its PAIR (ham, row) is below the query's bound T(q), the exact k-th smallest pair of all
// rows scanned before this launch, and goes to a candidate stream as a (query, key) record, key = ham << 32 | row.  The rows are scanned
// in GENERATIONS of geometrically growing ranges; after each one binary_select_kernel merges a query's records into its k best keys
// and the bound follows.  The order (ham, row) is total, so the bound admits exactly the rows that can still enter the list: with every
// row identical nothing after row k - 1 is admitted.  Results do not depend on the generation sizes, the stream's capacity or the order
// in which the atomics hand out stream slots: a query's records are unique keys, and they are sorted.
#include "index.h"

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace mvs {

namespace {

constexpr int BIN_MAX_D = 2048, BIN_MAX_K = 2048;
constexpr int BIN_PAD_DISTANCE = 2147483647;
constexpr int64_t BIN_QCHUNK = 16384;              // queries per pass: the stream of one 64-row generation then holds at most 2^20 records
constexpr int64_t BIN_MAX_STREAM = (int64_t)1 << 26; // records of the largest stream (12 bytes each); a generation that needs more is halved
constexpr int64_t BIN_GROWTH = 4;                  // a generation ends at 4 x the rows scanned before it
constexpr int64_t BIN_STAGE_ROWS = (int64_t)1 << 20; // rows one staging slot collects at most (their ids fill a slot of their own)
constexpr unsigned long long BIN_OPEN = ~0ull;     // no bound yet / an empty list entry: above every real key (ham <= 2048)
constexpr unsigned MAX_BLOCKS = 1u << 20;
constexpr uint32_t BIN_DEAD_LANE = 1u << 16;       // where a masked lane's distance starts: above d + 1, the largest radius the scan sees

__device__ __forceinline__ bool bin_sel_member(const SelectorDev &s, long long id) { // the membership rules of the remove_ids section
	if (s.kind == MVS_SEL_BITMAP) {
		const unsigned long long u = (unsigned long long)id; // (a negative id lands beyond every bitmap)
		if ((u >> 3) >= (unsigned long long)s.nbytes)
			return false;
		return (s.bitmap[u >> 3] >> (u & 7)) & 1;
	}
	long long lo = 0, hi = s.nids;
	while (lo < hi) {
		const long long mid = (lo + hi) >> 1;
		if (s.sorted_ids[mid] < id)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo < s.nids && s.sorted_ids[lo] == id;
}

// tiles [tile0, tile0 + ntiles) from the byte rows; rows at and beyond nrows are zero words
__global__ __launch_bounds__(256) void binary_pack_kernel(const uint8_t *__restrict__ codes, int code_size, int wpr, long long nrows, long long tile0,
                                                          long long ntiles, uint32_t *__restrict__ tiled) {
	const long long total = ntiles * wpr * 64;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const int lane = (int)(i & 63);
		const long long tw = i >> 6;
		const long long tile = tile0 + tw / wpr;
		const int w = (int)(tw % wpr);
		const long long row = tile * 64 + lane;
		uint32_t word = 0;
		if (row < nrows) {
			const uint8_t *p = codes + row * code_size;
			for (int b = 0; b < 4; ++b)
				if (4 * w + b < code_size)
					word |= (uint32_t)p[4 * w + b] << (8 * b);
		}
		tiled[(tile * wpr + w) * 64 + lane] = word;
	}
}

// queries as WP words each, zero beyond the code: the scan's inner loop has no tail
__global__ __launch_bounds__(256) void binary_pack_queries_kernel(const uint8_t *__restrict__ x, int code_size, int wp, long long nq,
                                                                  uint32_t *__restrict__ qw) {
	const long long total = (nq + 3) / 4 * 4 * wp; // (the scan reads whole groups of four queries: the pad is zero words)
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const long long q = i / wp;
		const int w = (int)(i - q * wp);
		uint32_t word = 0;
		for (int b = 0; b < 4; ++b)
			if (q < nq && 4 * w + b < code_size)
				word |= (uint32_t)x[q * code_size + 4 * w + b] << (8 * b);
		qw[i] = word;
	}
}

// the selector as one allowed-bit per row: allow[t] bit l = row 64 t + l exists and its id (ids[row], or the row number) is a member
__global__ __launch_bounds__(256) void binary_allow_kernel(SelectorDev sel, const long long *__restrict__ ids, long long n, long long ntiles,
                                                           unsigned long long *__restrict__ allow) {
	const int lane = threadIdx.x & 63;
	for (long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); tile < ntiles; tile += (long long)gridDim.x * 4) {
		const long long row = tile * 64 + lane;
		bool ok = false;
		if (row < n)
			ok = bin_sel_member(sel, ids ? ids[row] : row);
		const unsigned long long m = __ballot(ok);
		if (lane == 0)
			allow[tile] = m;
	}
}

// The admitted lanes of a wave take consecutive stream slots: one atomic per wave.  A record beyond the capacity is counted, not written.
__device__ __forceinline__ long long bin_stream_slot(bool adm, unsigned long long *cnt, int lane) {
	const unsigned long long m = __ballot(adm);
	if (!m)
		return -1;
	const int leader = __ffsll((long long)m) - 1;
	unsigned long long base = 0;
	if (lane == leader)
		base = atomicAdd(cnt, (unsigned long long)__popcll(m));
	base = __shfl(base, leader);
	return adm ? (long long)(base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull))) : -1;
}

// RANGE = false: admit (ham, row) < T[q]; record key = ham << 32 | row, recq = q.
// RANGE = true : admit ham < radius; record in range_collect's format: keys = q << 32 | row, vals = f32 bits of ham << 32 | row.
// Tiles [tile0, tile1) are dealt to the waves of grid.x; block y takes queries [y qb, (y + 1) qb).
template <int WP, bool RANGE>
__global__ __launch_bounds__(256) void binary_scan_kernel(const uint32_t *__restrict__ tiled, int wpr, const uint32_t *__restrict__ qw, int nq, int qb,
                                                          const unsigned long long *__restrict__ T, const unsigned long long *__restrict__ allow,
                                                          long long n, long long tile0, long long tile1, int radius,
                                                          unsigned long long *__restrict__ keys, unsigned long long *__restrict__ vals,
                                                          uint32_t *__restrict__ recq, unsigned long long *__restrict__ cnt, long long cap) {
	const int lane = threadIdx.x & 63;
	const int q0 = blockIdx.y * qb;
	const int q1 = min(q0 + qb, nq);
	for (long long tile = tile0 + (long long)blockIdx.x * 4 + (threadIdx.x >> 6); tile < tile1; tile += (long long)gridDim.x * 4) {
		const long long row = tile * 64 + lane;
		bool ok = row < n;
		if (allow)
			ok = ok && ((allow[tile] >> lane) & 1ull);
		if (!__ballot(ok))
			continue;
		// a lane whose row does not exist or is not allowed counts from beyond every distance: the tests on the distance below fail for it
		// without a mask of their own (a bound that is still open passes every lane; the pair test inside asks `ok`)
		const uint32_t bias = ok ? 0u : BIN_DEAD_LANE;
		uint32_t r[WP];
		const uint32_t *tp = tiled + tile * wpr * 64 + lane;
#pragma unroll
		for (int w = 0; w < WP; ++w)
			r[w] = w < wpr ? tp[w * 64] : 0u;
		for (int q = q0; q < q1; q += 4) { // four queries at a time: their scalar loads are in flight together (qw is padded to a multiple of 4)
			uint32_t ham[4] = {bias, bias, bias, bias};
			unsigned long long tq[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const uint32_t *qp = qw + (size_t)(q + j) * WP; // wave-uniform: scalar loads
				if (!RANGE)
					tq[j] = T[q + j]; // (padded like qw)
#pragma unroll
				for (int w = 0; w < WP; ++w)
					ham[j] += __popc(r[w] ^ qp[w]);
			}
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				if (q + j >= q1)
					break;
				if (RANGE) {
					const bool adm = (int)ham[j] < radius; // (radius <= d + 1 < BIN_DEAD_LANE: the host clamps it)
					if (__ballot(adm)) {
						const long long slot = bin_stream_slot(adm, cnt, lane);
						if (adm && slot < cap) {
							keys[slot] = ((unsigned long long)(unsigned)(q + j) << 32) | (unsigned)row;
							vals[slot] = ((unsigned long long)__float_as_uint((float)ham[j]) << 32) | (unsigned)row;
						}
					}
				} else {
					const unsigned long long t = tq[j];
					if (__ballot(ham[j] <= (uint32_t)(t >> 32))) { // the cheap test on the distance alone; the pair decides inside
						const unsigned long long key = ((unsigned long long)ham[j] << 32) | (unsigned)row;
						const bool adm = ok && key < t;
						const long long slot = bin_stream_slot(adm, cnt, lane);
						if (adm && slot < cap) {
							keys[slot] = key;
							recq[slot] = (uint32_t)(q + j);
						}
					}
				}
			}
		}
	}
}

__global__ __launch_bounds__(256) void binary_hist_kernel(const uint32_t *__restrict__ recq, long long n, unsigned *__restrict__ qcnt) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
		atomicAdd(&qcnt[recq[i]], 1u);
}
// records into their query's segment [qoff[q], qoff[q] + qcnt[q]); the order inside a segment is the atomics', the select sorts it away
__global__ __launch_bounds__(256) void binary_scatter_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ recq, long long n,
                                                             const unsigned *__restrict__ qoff, unsigned *__restrict__ qfill,
                                                             unsigned long long *__restrict__ seg) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
		const uint32_t q = recq[i];
		seg[qoff[q] + atomicAdd(&qfill[q], 1u)] = keys[i];
	}
}

// One workgroup per query: its k best keys so far and its segment's records, K2 at a time, through a bitonic sort of 2 K2 keys in LDS
// (K2 a power of two >= k); the K2 smallest stay.  Keys of one query are distinct, so the outcome is the k smallest keys in order.
__global__ __launch_bounds__(256) void binary_select_kernel(const unsigned long long *__restrict__ seg, const unsigned *__restrict__ qoff,
                                                            const unsigned *__restrict__ qcnt, int k, int K2, unsigned long long *__restrict__ best,
                                                            unsigned long long *__restrict__ T) {
	extern __shared__ unsigned long long bin_sh[];
	const int q = blockIdx.x, tid = threadIdx.x;
	const unsigned len = qcnt[q];
	if (len == 0)
		return;
	const unsigned long long *sp = seg + qoff[q];
	unsigned long long *bq = best + (size_t)q * k;
	const int S = 2 * K2;
	for (int i = tid; i < K2; i += 256)
		bin_sh[i] = i < k ? bq[i] : BIN_OPEN;
	for (unsigned c0 = 0; c0 < len; c0 += (unsigned)K2) {
		for (int i = tid; i < K2; i += 256)
			bin_sh[K2 + i] = c0 + (unsigned)i < len ? sp[c0 + (unsigned)i] : BIN_OPEN;
		__syncthreads();
		for (int size = 2; size <= S; size <<= 1)
			for (int stride = size >> 1; stride > 0; stride >>= 1) {
				for (int i = tid; i < S / 2; i += 256) {
					const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
					const bool up = (lo & size) == 0;
					const unsigned long long a = bin_sh[lo], b = bin_sh[hi];
					if ((a > b) == up) {
						bin_sh[lo] = b;
						bin_sh[hi] = a;
					}
				}
				__syncthreads();
			}
	}
	for (int i = tid; i < k; i += 256)
		bq[i] = bin_sh[i];
	if (tid == 0)
		T[q] = bin_sh[k - 1];
}

__global__ __launch_bounds__(256) void binary_fill_u64_kernel(unsigned long long *__restrict__ p, long long n, unsigned long long v) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
		p[i] = v;
}

// best keys -> (int32 distance, int64 label); an open entry is the padding (2147483647, -1)
__global__ __launch_bounds__(256) void binary_emit_kernel(const unsigned long long *__restrict__ best, long long total, const long long *__restrict__ ids,
                                                          int32_t *__restrict__ D, long long *__restrict__ I) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const unsigned long long key = best ? best[i] : BIN_OPEN;
		if (key == BIN_OPEN) {
			D[i] = BIN_PAD_DISTANCE;
			I[i] = -1;
		} else {
			const long long row = (long long)(unsigned)key;
			D[i] = (int32_t)(key >> 32);
			I[i] = ids ? ids[row] : row;
		}
	}
}

// reconstruct under IDMap: pos[j] = the LAST row whose id is i0 + j (-1: none)
__global__ __launch_bounds__(256) void binary_locate_kernel(const long long *__restrict__ ids, long long n, long long i0, long long ni,
                                                            long long *__restrict__ pos) {
	for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
		const long long id = ids[r];
		if (id >= i0 && id - i0 < ni)
			atomicMax(&pos[id - i0], r);
	}
}
__global__ __launch_bounds__(256) void binary_gather_kernel(const uint8_t *__restrict__ codes, int code_size, const long long *__restrict__ pos,
                                                            long long ni, uint8_t *__restrict__ out) {
	const long long total = ni * code_size;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const long long j = i / code_size;
		const long long r = pos[j];
		out[i] = r >= 0 ? codes[r * code_size + (i - j * code_size)] : (uint8_t)0;
	}
}

unsigned grid_for(long long n, int per_block = 256) {
	return (unsigned)std::max<long long>(1, std::min<long long>((n + per_block - 1) / per_block, MAX_BLOCKS));
}

// the scan has one instance per register-resident row length: the smallest of these that holds wpr words
int scan_words(int wpr) {
	static const int sizes[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64};
	for (int s : sizes)
		if (s >= wpr)
			return s;
	return 64;
}

struct ScanLaunch {
	const uint32_t *tiled;
	int wpr, wp;
	const uint32_t *qw;
	int nq;
	const unsigned long long *T, *allow;
	long long n, tile0, tile1;
	int radius;
	unsigned long long *keys, *vals;
	uint32_t *recq;
	unsigned long long *cnt;
	long long cap;
};

template <bool RANGE>
void launch_scan(const ScanLaunch &a, hipStream_t st) {
	const long long ntiles = a.tile1 - a.tile0;
	if (ntiles <= 0 || a.nq <= 0)
		return;
	const long long bx = std::min<long long>((ntiles + 3) / 4, 8192);
	// queries per block: as many as keep a few thousand blocks in flight, so that a tile's words are loaded once per 64 .. 1024 queries
	long long qb = std::max<long long>(64, std::min<long long>(1024, (long long)a.nq * bx / 2048));
	qb = std::min<long long>(qb / 4 * 4, a.nq); // (whole groups of four, or the one block that takes every query)
	const dim3 grid((unsigned)bx, (unsigned)((a.nq + qb - 1) / qb));
#define MVS_BIN_SCAN(W)                                                                                                                          \
	case W:                                                                                                                                      \
		hipLaunchKernelGGL((binary_scan_kernel<W, RANGE>), grid, dim3(256), 0, st, a.tiled, a.wpr, a.qw, a.nq, (int)qb, a.T, a.allow, a.n, a.tile0, \
		                   a.tile1, a.radius, a.keys, a.vals, a.recq, a.cnt, a.cap);                                                            \
		break;
	switch (a.wp) {
		MVS_BIN_SCAN(1)
		MVS_BIN_SCAN(2)
		MVS_BIN_SCAN(3)
		MVS_BIN_SCAN(4)
		MVS_BIN_SCAN(6)
		MVS_BIN_SCAN(8)
		MVS_BIN_SCAN(12)
		MVS_BIN_SCAN(16)
		MVS_BIN_SCAN(24)
		MVS_BIN_SCAN(32)
		MVS_BIN_SCAN(48)
		MVS_BIN_SCAN(64)
	default:
		throw_faiss("mvs::launch_scan", __FILE__, "no scan instance for %d words per row", a.wp);
	}
#undef MVS_BIN_SCAN
	MVS_HIP(hipGetLastError());
}

const char *const FN_FACTORY = "faiss::IndexBinary* faiss::index_binary_factory(int, const char*)";
const char *const FN_READ = "faiss::IndexBinary* faiss::read_index_binary(const char*, int)";

} // namespace

// ------------------------------------------------------------------------------------------------------------------------------ the index

class BinaryIndex {
public:
	int d, code_size, wpr;
	bool idmap, idmap2;
	int64_t ntotal = 0; // every row added, staged ones included
	int device = 0;
	hipStream_t stream = nullptr;

	BinaryIndex(int d_, bool idmap_, bool idmap2_) : d(d_), code_size(d_ / 8), wpr((d_ + 31) / 32), idmap(idmap_), idmap2(idmap2_) {
		int ndev = 0;
		const hipError_t e = hipGetDeviceCount(&ndev);
		if (e != hipSuccess || ndev <= 0)
			throw_faiss("mvs::BinaryIndex::BinaryIndex", __FILE__,
			            "no MI355X (gfx950) device is usable (%s): the MI355X vector-search path has no CPU fallback",
			            e == hipSuccess ? "device count 0" : hipGetErrorString(e));
		const char *env = getenv("MVS_DEVICE");
		device = env ? atoi(env) : 0;
		if (device < 0 || device >= ndev)
			throw_faiss("mvs::BinaryIndex::BinaryIndex", __FILE__, "Invalid GPU device %d", device);
		MVS_HIP(hipSetDevice(device));
		MVS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
	}
	~BinaryIndex() {
		(void)hipSetDevice(device);
		if (stream) {
			(void)hipStreamSynchronize(stream);
			(void)hipStreamDestroy(stream);
		}
	}
	BinaryIndex(const BinaryIndex &) = delete;
	BinaryIndex &operator=(const BinaryIndex &) = delete;

	void use_device() const {
		MVS_HIP(hipSetDevice(device));
	}
	void reset() {
		use_device();
		MVS_HIP(hipStreamSynchronize(stream));
		pend_slot = -1, pend_rows = 0, pend_bytes = 0;
		dev_rows = 0, ntotal = 0;
	}

	// ---- add: small adds collect in a pinned slot (and their ids in another) and reach the device once per slot, as FlatIndex's do
	void add(int64_t n, const uint8_t *x, const int64_t *ids) {
		use_device();
		if (n <= 0)
			return;
		check_rows(n);
		const size_t bytes = (size_t)n * code_size;
		if (bytes > PinnedRing::SLOT_BYTES / 2 || n > BIN_STAGE_ROWS / 2) { // a large add goes straight to the device
			flush();
			grow(dev_rows + n);
			MVS_HIP(hipMemcpyAsync(codes_.get() + (size_t)dev_rows * code_size, x, bytes, hipMemcpyHostToDevice, stream));
			if (idmap)
				MVS_HIP(hipMemcpyAsync(ids_.get() + dev_rows, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, stream));
			pack_new_rows(n);
			MVS_HIP(hipStreamSynchronize(stream)); // (the caller's rows are pageable memory: they are read before the call returns)
			return;
		}
		if (pend_slot >= 0 && (pend_bytes + bytes > PinnedRing::SLOT_BYTES || pend_rows + n > BIN_STAGE_ROWS))
			flush();
		if (pend_slot < 0) {
			pend_slot = add_ring.acquire(PinnedRing::SLOT_BYTES);
			if (idmap)
				pend_id_slot = id_ring.acquire((size_t)BIN_STAGE_ROWS * sizeof(int64_t));
			pend_bytes = 0, pend_rows = 0;
		}
		memcpy((char *)add_ring.buf[pend_slot] + pend_bytes, x, bytes);
		if (idmap)
			memcpy((int64_t *)id_ring.buf[pend_id_slot] + pend_rows, ids, (size_t)n * sizeof(int64_t));
		pend_bytes += bytes, pend_rows += n;
		ntotal += n;
	}
	// device rows (and ids): ordered after `st`, done on the index's stream, and `st` waits for it
	void add_device(int64_t n, const uint8_t *d_x, const int64_t *d_ids, hipStream_t st) {
		use_device();
		if (n <= 0)
			return;
		check_rows(n);
		flush();
		stream_wait(stream, st);
		grow(dev_rows + n);
		MVS_HIP(hipMemcpyAsync(codes_.get() + (size_t)dev_rows * code_size, d_x, (size_t)n * code_size, hipMemcpyDeviceToDevice, stream));
		if (idmap)
			MVS_HIP(hipMemcpyAsync(ids_.get() + dev_rows, d_ids, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
		pack_new_rows(n);
		stream_wait(st, stream);
	}
	// every reader calls this first: the staged rows reach the device (on `stream`)
	void flush() {
		if (pend_slot < 0)
			return;
		const int64_t n = pend_rows;
		grow(dev_rows + n);
		MVS_HIP(hipMemcpyAsync(codes_.get() + (size_t)dev_rows * code_size, add_ring.buf[pend_slot], pend_bytes, hipMemcpyHostToDevice, stream));
		add_ring.release(pend_slot, stream);
		if (idmap) {
			MVS_HIP(hipMemcpyAsync(ids_.get() + dev_rows, id_ring.buf[pend_id_slot], (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, stream));
			id_ring.release(pend_id_slot, stream);
		}
		pend_slot = -1, pend_rows = 0, pend_bytes = 0;
		pack_new_rows(n);
		++add_flushes;
	}

	// ---- search, device pointers, on the index's stream.  mapped: labels and the selector's ids are id_map[row] (the IDMap wrapper's view)
	void search_device(int64_t nq, const uint8_t *d_x, int64_t k, int32_t *d_D, int64_t *d_I, const mvs_search_params *params, bool mapped) {
		use_device();
		check_k(k);
		if (nq <= 0)
			return;
		flush();
		scan_launches = 0, candidates = 0;
		const long long *map = mapped ? (const long long *)ids_.get() : nullptr;
		if (dev_rows == 0) {
			hipLaunchKernelGGL(binary_emit_kernel, dim3(grid_for(nq * k)), dim3(256), 0, stream, (const unsigned long long *)nullptr,
			                   (long long)(nq * k), map, d_D, (long long *)d_I);
			MVS_HIP(hipGetLastError());
			return;
		}
		const int64_t n = dev_rows, ntiles = (n + 63) / 64;
		const unsigned long long *allow = build_allow(params, map, n);
		const int wp = scan_words(wpr);
		int K2 = 256;
		while (K2 < k)
			K2 <<= 1;
		// rows examined before the first bound exists: at least k of them, whole tiles
		const int64_t first = (std::max<int64_t>(first_rows, k) + 63) / 64 * 64;
		for (int64_t q0 = 0; q0 < nq; q0 += BIN_QCHUNK) {
			const int64_t nc = std::min(BIN_QCHUNK, nq - q0);
			ws_q.reserve((size_t)(nc + 4) * wp * 4);
			ws_best.reserve((size_t)nc * k * 8);
			ws_ctl.reserve(64 + (size_t)nc * 8 + 3 * (size_t)(nc + 1) * 4 + 64); // (the scan reads the bounds of whole groups of four queries)
			unsigned long long *d_cnt = (unsigned long long *)ws_ctl.p;
			unsigned long long *d_T = (unsigned long long *)((char *)ws_ctl.p + 64);
			unsigned *d_qcnt = (unsigned *)(d_T + nc + 4), *d_qoff = d_qcnt + (nc + 1), *d_qfill = d_qoff + (nc + 1);
			hipLaunchKernelGGL(binary_pack_queries_kernel, dim3(grid_for(nc * wp)), dim3(256), 0, stream, d_x + (size_t)q0 * code_size, code_size, wp,
			                   (long long)nc, (uint32_t *)ws_q.p);
			hipLaunchKernelGGL(binary_fill_u64_kernel, dim3(grid_for(nc * k)), dim3(256), 0, stream, (unsigned long long *)ws_best.p, (long long)(nc * k),
			                   BIN_OPEN);
			hipLaunchKernelGGL(binary_fill_u64_kernel, dim3(grid_for(nc + 4)), dim3(256), 0, stream, d_T, (long long)(nc + 4), BIN_OPEN);
			MVS_HIP(hipGetLastError());
			int64_t cap = stream_cap > 0 ? stream_cap
			                             : std::min<int64_t>(BIN_MAX_STREAM, std::max<int64_t>({nc * std::min<int64_t>(first, n), nc * k * 4, (int64_t)65536}));
			int64_t a = 0, gen_end = first;
			while (a < n) { // one generation: rows [a, b)
				int64_t b = std::min(n, gen_end);
				unsigned long long cnt = 0;
				for (;;) {
					ws_keys.reserve((size_t)cap * 8);
					ws_recq.reserve((size_t)cap * 4);
					MVS_HIP(hipMemsetAsync(d_cnt, 0, 8, stream));
					ScanLaunch s;
					memset(&s, 0, sizeof s);
					s.tiled = tiled_.get(), s.wpr = wpr, s.wp = wp, s.qw = (const uint32_t *)ws_q.p, s.nq = (int)nc, s.T = d_T, s.allow = allow;
					s.n = n, s.tile0 = a / 64, s.tile1 = std::min<int64_t>((b + 63) / 64, ntiles);
					s.keys = (unsigned long long *)ws_keys.p, s.recq = (uint32_t *)ws_recq.p, s.cnt = d_cnt, s.cap = cap;
					launch_scan<false>(s, stream);
					++scan_launches;
					MVS_HIP(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, stream));
					MVS_HIP(hipStreamSynchronize(stream));
					if ((int64_t)cnt <= cap)
						break;
					// the stream was too small: nothing of this generation is kept, it runs again with enough room -- or, where even the
					// largest stream would not hold it, as a shorter generation (the next one then scans under a tighter bound)
					++rescans;
					if ((int64_t)cnt <= BIN_MAX_STREAM) {
						cap = (int64_t)cnt; // (the scan is deterministic under a fixed bound: the count is exact)
						continue;
					}
					if (b - a <= 64)
						throw_faiss("mvs::BinaryIndex::search", __FILE__, "%llu candidates of one 64-row generation exceed the stream's %lld entries",
						            cnt, (long long)BIN_MAX_STREAM);
					b = a + std::max<int64_t>(64, (b - a) / 2 / 64 * 64);
					cap = std::max(cap, std::min<int64_t>(BIN_MAX_STREAM, nc * 64));
				}
				candidates += (int64_t)cnt;
				if (cnt > 0)
					merge_generation((int64_t)cnt, nc, (int)k, K2, d_T, d_qcnt, d_qoff, d_qfill);
				a = b;
				gen_end = b * BIN_GROWTH;
			}
			hipLaunchKernelGGL(binary_emit_kernel, dim3(grid_for(nc * k)), dim3(256), 0, stream, (const unsigned long long *)ws_best.p, (long long)(nc * k),
			                   map, d_D + (size_t)q0 * k, (long long *)d_I + (size_t)q0 * k);
			MVS_HIP(hipGetLastError());
		}
	}
	void search(int64_t nq, const uint8_t *x, int64_t k, int32_t *D, int64_t *I, const mvs_search_params *params, bool mapped) {
		use_device();
		check_k(k);
		if (nq <= 0)
			return;
		ws_hx.reserve((size_t)nq * code_size);
		ws_hD.reserve((size_t)nq * k * 4);
		ws_hI.reserve((size_t)nq * k * 8);
		MVS_HIP(hipMemcpyAsync(ws_hx.p, x, (size_t)nq * code_size, hipMemcpyHostToDevice, stream));
		search_device(nq, (const uint8_t *)ws_hx.p, k, (int32_t *)ws_hD.p, (int64_t *)ws_hI.p, params, mapped);
		MVS_HIP(hipMemcpyAsync(D, ws_hD.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, stream));
		MVS_HIP(hipMemcpyAsync(I, ws_hI.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, stream));
		MVS_HIP(hipStreamSynchronize(stream));
	}

	// ---- range_search: the same scan with the fixed test ham < radius into range_collect's stream; its sort by (query, row), lims and labels
	void range_search(int64_t nq, const uint8_t *x, int radius, const mvs_search_params *params, bool mapped, RangeResult &out) {
		use_device();
		flush();
		out.clear(nq);
		if (nq <= 0 || dev_rows == 0 || radius <= 0)
			return;
		const int64_t n = dev_rows, ntiles = (n + 63) / 64;
		if (n >= ((int64_t)1 << 32))
			throw_faiss("mvs::BinaryIndex::range_search", __FILE__, "an index of %lld rows is beyond the 2^32 rows a range search numbers", (long long)n);
		const long long *map = mapped ? (const long long *)ids_.get() : nullptr;
		const unsigned long long *allow = build_allow(params, map, n);
		const int wp = scan_words(wpr);
		range_work.stream_cap = stream_cap;
		const int64_t chunk = 65536;
		for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
			const int64_t nc = std::min(chunk, nq - q0);
			ws_hx.reserve((size_t)nc * code_size);
			ws_q.reserve((size_t)(nc + 4) * wp * 4);
			MVS_HIP(hipMemcpyAsync(ws_hx.p, x + (size_t)q0 * code_size, (size_t)nc * code_size, hipMemcpyHostToDevice, stream));
			hipLaunchKernelGGL(binary_pack_queries_kernel, dim3(grid_for(nc * wp)), dim3(256), 0, stream, (const uint8_t *)ws_hx.p, code_size, wp,
			                   (long long)nc, (uint32_t *)ws_q.p);
			MVS_HIP(hipGetLastError());
			RangeScan rs;
			memset(&rs, 0, sizeof rs);
			rs.nq = nc, rs.nrows = n, rs.radius = (float)radius;
			const int64_t before = range_work.rescans;
			range_collect(range_work, rs, [&](const RangeScan &sc) {
				ScanLaunch s;
				memset(&s, 0, sizeof s);
				s.tiled = tiled_.get(), s.wpr = wpr, s.wp = wp, s.qw = (const uint32_t *)ws_q.p, s.nq = (int)nc, s.allow = allow;
				s.n = n, s.tile0 = 0, s.tile1 = ntiles, s.radius = std::min(radius, d + 1); // (ham <= d: a larger radius admits nothing more)
				s.keys = sc.keys, s.vals = sc.vals, s.cnt = sc.cnt, s.cap = sc.cap;
				launch_scan<true>(s, stream);
			}, q0, nullptr, mapped ? ids_.get() : nullptr, 0, out, stream);
			rescans += range_work.rescans - before;
		}
	}

	// ---- reconstruct_n: positions i0 .. i0 + ni - 1 (bare), or the external keys i0 .. i0 + ni - 1, each of which must exist (IDMap)
	void reconstruct_n(int64_t i0, int64_t ni, uint8_t *out, bool mapped, bool single) {
		use_device();
		flush();
		if (ni < 0)
			throw_faiss("virtual void faiss::IndexBinary::reconstruct_n(...) const", "faiss/IndexBinary.cpp",
			            "Error: 'ni == 0 || (i0 >= 0 && i0 + ni <= ntotal)' failed");
		if (ni == 0)
			return;
		ws_hI.reserve((size_t)ni * 8);
		ws_hx.reserve((size_t)ni * code_size);
		long long *d_pos = (long long *)ws_hI.p;
		if (!mapped) {
			if (i0 < 0 || i0 + ni > dev_rows)
				throw_faiss(single ? "virtual void faiss::IndexBinaryFlat::reconstruct(faiss::idx_t, uint8_t*) const"
				                   : "virtual void faiss::IndexBinary::reconstruct_n(...) const",
				            "faiss/IndexBinary.cpp", "Error: 'ni == 0 || (i0 >= 0 && i0 + ni <= ntotal)' failed: rows [%lld, %lld) outside [0, %lld)",
				            (long long)i0, (long long)(i0 + ni), (long long)dev_rows);
			MVS_HIP(hipMemcpyAsync(out, codes_.get() + (size_t)i0 * code_size, (size_t)ni * code_size, hipMemcpyDeviceToHost, stream));
			MVS_HIP(hipStreamSynchronize(stream));
			return;
		}
		MVS_HIP(hipMemsetAsync(d_pos, 0xFF, (size_t)ni * 8, stream));
		if (dev_rows > 0)
			hipLaunchKernelGGL(binary_locate_kernel, dim3(grid_for(dev_rows)), dim3(256), 0, stream, (const long long *)ids_.get(), (long long)dev_rows,
			                   (long long)i0, (long long)ni, d_pos);
		hipLaunchKernelGGL(binary_gather_kernel, dim3(grid_for(ni * code_size)), dim3(256), 0, stream, (const uint8_t *)codes_.get(), code_size,
		                   (const long long *)d_pos, (long long)ni, (uint8_t *)ws_hx.p);
		MVS_HIP(hipGetLastError());
		std::vector<long long> pos((size_t)ni);
		MVS_HIP(hipMemcpyAsync(pos.data(), d_pos, (size_t)ni * 8, hipMemcpyDeviceToHost, stream));
		MVS_HIP(hipMemcpyAsync(out, ws_hx.p, (size_t)ni * code_size, hipMemcpyDeviceToHost, stream));
		MVS_HIP(hipStreamSynchronize(stream));
		for (int64_t j = 0; j < ni; ++j)
			if (pos[(size_t)j] < 0)
				throw_faiss("virtual void faiss::IndexBinaryIDMap::reconstruct(faiss::idx_t, uint8_t*) const", "faiss/IndexBinaryIDMap.cpp",
				            "key not found: %lld", (long long)(i0 + j));
	}

	// ---- host image (write_index_binary): the byte rows and, under IDMap, the id map
	void to_host(std::vector<uint8_t> &rows, std::vector<int64_t> &ids) {
		use_device();
		flush();
		rows.resize((size_t)dev_rows * code_size);
		ids.resize(idmap ? (size_t)dev_rows : 0);
		if (dev_rows > 0) {
			MVS_HIP(hipMemcpyAsync(rows.data(), codes_.get(), rows.size(), hipMemcpyDeviceToHost, stream));
			if (idmap)
				MVS_HIP(hipMemcpyAsync(ids.data(), ids_.get(), ids.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
		}
		MVS_HIP(hipStreamSynchronize(stream));
	}

	bool set_option(const char *key, int64_t v) {
		if (!strcmp(key, "binary_first_rows")) {
			if (v < 1)
				throw_faiss("mvs::BinaryIndex::set_option", __FILE__, "binary_first_rows = %lld: at least 1", (long long)v);
			first_rows = v;
			return true;
		}
		if (!strcmp(key, "binary_stream_cap")) {
			if (v < 0 || v > BIN_MAX_STREAM)
				throw_faiss("mvs::BinaryIndex::set_option", __FILE__, "binary_stream_cap = %lld: 0 (automatic) .. %lld", (long long)v,
				            (long long)BIN_MAX_STREAM);
			stream_cap = v;
			return true;
		}
		return false;
	}
	bool get_stat(const char *name, int64_t *v) const {
		if (!strcmp(name, "binary_scan_launches"))
			*v = scan_launches;
		else if (!strcmp(name, "binary_candidates"))
			*v = candidates;
		else if (!strcmp(name, "binary_rescans"))
			*v = rescans;
		else if (!strcmp(name, "binary_add_flushes"))
			*v = add_flushes;
		else if (!strcmp(name, "device_bytes_live")) // of the process, as mvs_index_get_stat's: device memory held through csrc/dev_mem.h's owners
			*v = g_dev_bytes_live.load();
		else
			return false;
		return true;
	}

private:
	DevBlock<uint8_t> codes_;  // [cap][code_size]
	DevBlock<uint32_t> tiled_; // [cap / 64][wpr][64]
	DevBlock<int64_t> ids_;    // [cap] (IDMap)
	int64_t cap = 0, dev_rows = 0; // rows allocated (whole tiles) / rows on the device
	PinnedRing add_ring, id_ring;
	int pend_slot = -1, pend_id_slot = -1;
	size_t pend_bytes = 0;
	int64_t pend_rows = 0;
	int64_t first_rows = 256, stream_cap = 0;                                  // options binary_first_rows / binary_stream_cap
	int64_t scan_launches = 0, candidates = 0, rescans = 0, add_flushes = 0; // of the last search (the first two) / of the index's life
	DevBuf ws_q, ws_best, ws_ctl, ws_keys, ws_recq, ws_seg, ws_temp, ws_allow, ws_hx, ws_hD, ws_hI;
	SelectorHolder selector;
	RangeWork range_work;

	static void check_k(int64_t k) {
		if (k <= 0)
			throw_faiss("virtual void faiss::IndexBinaryFlat::search(...) const", "faiss/IndexBinaryFlat.cpp", "Error: 'k > 0' failed");
		if (k > BIN_MAX_K)
			throw_faiss("mvs::BinaryIndex::search", __FILE__, "k = %lld is beyond the largest k the binary index serves on the MI355X path (%d)",
			            (long long)k, BIN_MAX_K);
	}
	void check_rows(int64_t n) const {
		if (ntotal + n > ((int64_t)1 << 31) - 1024)
			throw_faiss("mvs::BinaryIndex::add", __FILE__, "%lld rows are beyond the 2^31 - 1024 rows a binary index holds", (long long)(ntotal + n));
	}
	void grow(int64_t need) {
		if (need <= cap)
			return;
		const int64_t ncap = (std::max<int64_t>({need, cap * 2, (int64_t)4096}) + 63) / 64 * 64;
		// all new arrays before any old one goes: a failure leaves the index as it was
		DevBlock<uint8_t> nc((size_t)ncap * code_size);
		DevBlock<uint32_t> nt;
		DevBlock<int64_t> ni;
		try {
			nt = DevBlock<uint32_t>((size_t)ncap * wpr);
			if (idmap)
				ni = DevBlock<int64_t>((size_t)ncap);
		} catch (...) {
			throw_faiss("mvs::BinaryIndex::grow", __FILE__, "out of device memory for %lld rows of %d bits", (long long)ncap, d);
		}
		if (dev_rows > 0) {
			const int64_t tiles = (dev_rows + 63) / 64;
			MVS_HIP(hipMemcpyAsync(nc.get(), codes_.get(), (size_t)dev_rows * code_size, hipMemcpyDeviceToDevice, stream));
			MVS_HIP(hipMemcpyAsync(nt.get(), tiled_.get(), (size_t)tiles * wpr * 256, hipMemcpyDeviceToDevice, stream));
			if (idmap)
				MVS_HIP(hipMemcpyAsync(ni.get(), ids_.get(), (size_t)dev_rows * 8, hipMemcpyDeviceToDevice, stream));
		}
		MVS_HIP(hipStreamSynchronize(stream)); // (nothing reads the old stores any more)
		codes_ = std::move(nc), tiled_ = std::move(nt), ids_ = std::move(ni), cap = ncap;
	}
	// rows [dev_rows, dev_rows + n) are in `codes`: their tiles (the first one may be half old) are built again from the byte rows
	void pack_new_rows(int64_t n) {
		const int64_t tile0 = dev_rows / 64, tile1 = (dev_rows + n + 63) / 64;
		hipLaunchKernelGGL(binary_pack_kernel, dim3(grid_for((tile1 - tile0) * wpr * 64)), dim3(256), 0, stream, (const uint8_t *)codes_.get(), code_size, wpr,
		                   (long long)(dev_rows + n), (long long)tile0, (long long)(tile1 - tile0), tiled_.get());
		MVS_HIP(hipGetLastError());
		dev_rows += n;
		ntotal = dev_rows;
	}
	const unsigned long long *build_allow(const mvs_search_params *params, const long long *map, int64_t n) {
		if (!params || params->sel_kind == MVS_SEL_NONE)
			return nullptr;
		const SelectorDev sel = selector.upload(params, IdDomain::rows(0, n, (const int64_t *)map), stream); // (the allow mask tests map[row], or the row)
		const int64_t ntiles = (n + 63) / 64;
		ws_allow.reserve((size_t)ntiles * 8);
		hipLaunchKernelGGL(binary_allow_kernel, dim3(grid_for(ntiles, 4)), dim3(256), 0, stream, sel, map, (long long)n, (long long)ntiles,
		                   (unsigned long long *)ws_allow.p);
		MVS_HIP(hipGetLastError());
		return (const unsigned long long *)ws_allow.p;
	}
	// the records of one generation join their queries' lists: per-query counts, offsets, segments, the select; the bound follows
	void merge_generation(int64_t cnt, int64_t nc, int k, int K2, unsigned long long *d_T, unsigned *d_qcnt, unsigned *d_qoff, unsigned *d_qfill) {
		ws_seg.reserve((size_t)cnt * 8);
		MVS_HIP(hipMemsetAsync(d_qcnt, 0, (size_t)(nc + 1) * 4, stream));
		MVS_HIP(hipMemsetAsync(d_qfill, 0, (size_t)(nc + 1) * 4, stream));
		hipLaunchKernelGGL(binary_hist_kernel, dim3(grid_for(cnt)), dim3(256), 0, stream, (const uint32_t *)ws_recq.p, (long long)cnt, d_qcnt);
		size_t temp_bytes = 0;
		MVS_HIP(rocprim::exclusive_scan(nullptr, temp_bytes, d_qcnt, d_qoff, 0u, (size_t)(nc + 1), rocprim::plus<unsigned>(), stream));
		ws_temp.reserve(std::max<size_t>(temp_bytes, 16));
		MVS_HIP(rocprim::exclusive_scan(ws_temp.p, temp_bytes, d_qcnt, d_qoff, 0u, (size_t)(nc + 1), rocprim::plus<unsigned>(), stream));
		hipLaunchKernelGGL(binary_scatter_kernel, dim3(grid_for(cnt)), dim3(256), 0, stream, (const unsigned long long *)ws_keys.p,
		                   (const uint32_t *)ws_recq.p, (long long)cnt, (const unsigned *)d_qoff, d_qfill, (unsigned long long *)ws_seg.p);
		hipLaunchKernelGGL(binary_select_kernel, dim3((unsigned)nc), dim3(256), (size_t)2 * K2 * 8, stream, (const unsigned long long *)ws_seg.p,
		                   (const unsigned *)d_qoff, (const unsigned *)d_qcnt, k, K2, (unsigned long long *)ws_best.p, d_T);
		MVS_HIP(hipGetLastError());
	}
};

// ------------------------------------------------------------------------------------------------------------------------------ factory

static void check_binary_d(int d, const char *fn, const std::string &what) {
	if (d <= 0 || d % 8 != 0)
		throw_faiss(fn, "faiss/IndexBinary.cpp", "Error: 'd %% 8 == 0' failed (d = %d)", d);
	if (d > BIN_MAX_D)
		throw_faiss(fn, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s with d = %d (at most %d bits)",
		            what.c_str(), d, BIN_MAX_D);
}

static BinaryIndex *binary_factory(int d, const char *description) {
	const std::string full = description ? description : "";
	std::string desc = full;
	bool idmap = false, idmap2 = false;
	if (desc.rfind("IDMap2,", 0) == 0)
		idmap = idmap2 = true, desc = desc.substr(7);
	else if (desc.rfind("IDMap,", 0) == 0)
		idmap = true, desc = desc.substr(6);
	if (desc == "BFlat") {
		check_binary_d(d, FN_FACTORY, full);
		return new BinaryIndex(d, idmap, idmap2);
	}
	if (desc.rfind("BIVF", 0) == 0 || desc.rfind("BHNSW", 0) == 0 || desc.rfind("BHash", 0) == 0)
		throw_faiss(FN_FACTORY, "faiss/index_factory.cpp", "This index type is not implemented on the MI355X path yet: %s", full.c_str());
	throw_faiss(FN_FACTORY, "faiss/index_factory.cpp", "could not parse index string %s", full.c_str());
}

// ------------------------------------------------------------------------------------------------------------------------------ files
// fourcc "IBxF": int32 d, int32 code_size, int64 ntotal, uint8 is_trained, int32 metric_type, then the codes as a vector (uint64 count of
// bytes, the bytes).  "IBMp" / "IBM2": the same header, the sub-index's image, id_map as uint64 count + int64s.  The bytes restate FAISS's
// impl/index_write.cpp FROM MEMORY and are not pinned against a FAISS build (as for csrc/index_io.hip).

namespace {

uint32_t bin_fourcc(const char *s) {
	return (uint32_t)(uint8_t)s[0] | ((uint32_t)(uint8_t)s[1] << 8) | ((uint32_t)(uint8_t)s[2] << 16) | ((uint32_t)(uint8_t)s[3] << 24);
}
struct BinWriter {
	FILE *f;
	const char *name;
	void bytes(const void *p, size_t n) {
		if (n && fwrite(p, 1, n, f) != n)
			throw_faiss("faiss::FileIOWriter::operator()", "faiss/impl/io.cpp", "write error in %s: %s", name, strerror(errno));
	}
	template <class T>
	void one(const T &v) {
		bytes(&v, sizeof v);
	}
};
struct BinReader {
	FILE *f;
	const char *name;
	void bytes(void *p, size_t n, const char *what) {
		const long at = ftell(f);
		const size_t got = n ? fread(p, 1, n, f) : 0;
		if (got != n)
			throw_faiss(FN_READ, "faiss/impl/index_read.cpp", "file %s is truncated: %s wants %llu bytes at offset %ld, the file has %llu", name, what,
			            (unsigned long long)n, at, (unsigned long long)got);
	}
	template <class T>
	void one(T &v, const char *what) {
		bytes(&v, sizeof v, what);
	}
};
struct BinHeader {
	int32_t d = 0, code_size = 0, metric = 1;
	int64_t ntotal = 0;
	uint8_t is_trained = 1;
};
void write_header(BinWriter &w, const char *cc, const BinHeader &h) {
	w.one(bin_fourcc(cc));
	w.one(h.d);
	w.one(h.code_size);
	w.one(h.ntotal);
	w.one(h.is_trained);
	w.one(h.metric);
}
void read_header(BinReader &r, BinHeader &h) {
	r.one(h.d, "d");
	r.one(h.code_size, "code_size");
	r.one(h.ntotal, "ntotal");
	r.one(h.is_trained, "is_trained");
	r.one(h.metric, "metric_type");
	if (h.d <= 0 || h.d % 8 != 0)
		throw_faiss(FN_READ, "faiss/impl/index_read.cpp", "Error: 'd %% 8 == 0' failed (d = %d)", h.d);
	if (h.code_size != h.d / 8)
		throw_faiss(FN_READ, "faiss/impl/index_read.cpp", "code_size = %d does not belong to d = %d (d / 8 = %d)", h.code_size, h.d, h.d / 8);
	if (h.ntotal < 0)
		throw_faiss(FN_READ, "faiss/impl/index_read.cpp", "ntotal = %lld is negative", (long long)h.ntotal);
	check_binary_d(h.d, FN_READ, "a binary index file");
}
uint32_t read_fourcc(BinReader &r, char *txt) {
	uint32_t cc = 0;
	r.one(cc, "the fourcc");
	for (int i = 0; i < 4; ++i) {
		const char c = (char)((cc >> (8 * i)) & 0xff);
		txt[i] = c >= 32 && c <= 126 ? c : '?';
	}
	txt[4] = 0;
	return cc;
}
void read_flat_body(BinReader &r, const BinHeader &h, std::vector<uint8_t> &rows) {
	uint64_t nbytes = 0;
	r.one(nbytes, "the size of the codes");
	if (nbytes != (uint64_t)h.ntotal * (uint64_t)h.code_size)
		throw_faiss(FN_READ, "faiss/impl/index_read.cpp", "the codes hold %llu bytes where ntotal x code_size = %lld x %d = %llu",
		            (unsigned long long)nbytes, (long long)h.ntotal, h.code_size, (unsigned long long)((uint64_t)h.ntotal * (uint64_t)h.code_size));
	rows.resize((size_t)nbytes);
	r.bytes(rows.data(), rows.size(), "the codes");
}

} // namespace

static void write_binary_file(BinaryIndex *ix, const char *filename) {
	std::vector<uint8_t> rows;
	std::vector<int64_t> ids;
	ix->to_host(rows, ids);
	FILE *f = fopen(filename, "wb");
	if (!f)
		throw_faiss("faiss::FileIOWriter::FileIOWriter(const char*)", "faiss/impl/io.cpp", "could not open %s for writing: %s", filename,
		            strerror(errno));
	BinWriter w {f, filename};
	try {
		BinHeader h;
		h.d = ix->d, h.code_size = ix->code_size, h.ntotal = (int64_t)(rows.size() / (size_t)ix->code_size);
		if (ix->idmap)
			write_header(w, ix->idmap2 ? "IBM2" : "IBMp", h);
		write_header(w, "IBxF", h);
		w.one((uint64_t)rows.size());
		w.bytes(rows.data(), rows.size());
		if (ix->idmap) {
			w.one((uint64_t)ids.size());
			w.bytes(ids.data(), ids.size() * sizeof(int64_t));
		}
	} catch (...) {
		fclose(f);
		throw;
	}
	if (fclose(f) != 0)
		throw_faiss("faiss::FileIOWriter::~FileIOWriter()", "faiss/impl/io.cpp", "file %s close error: %s", filename, strerror(errno));
}

static BinaryIndex *read_binary_file(const char *filename) {
	FILE *f = fopen(filename, "rb");
	if (!f)
		throw_faiss("faiss::FileIOReader::FileIOReader(const char*)", "faiss/impl/io.cpp", "could not open %s for reading: %s", filename,
		            strerror(errno));
	BinReader r {f, filename};
	BinHeader h, hs;
	std::vector<uint8_t> rows;
	std::vector<int64_t> ids;
	bool idmap = false, idmap2 = false;
	try {
		char txt[5];
		uint32_t cc = read_fourcc(r, txt);
		if (cc == bin_fourcc("IBMp") || cc == bin_fourcc("IBM2")) {
			idmap = true, idmap2 = cc == bin_fourcc("IBM2");
			read_header(r, h);
			cc = read_fourcc(r, txt);
			if (cc != bin_fourcc("IBxF"))
				throw_faiss(FN_READ, "faiss/impl/index_read.cpp",
				            "Index type 0x%08x (\"%s\") under IndexBinaryIDMap is not implemented on the MI355X path (\"IBxF\" only)", cc, txt);
			read_header(r, hs);
			if (hs.d != h.d || hs.ntotal != h.ntotal)
				throw_faiss(FN_READ, "faiss/impl/index_read.cpp", "the sub-index (d = %d, ntotal = %lld) does not belong to its IndexBinaryIDMap (d = %d, ntotal = %lld)",
				            hs.d, (long long)hs.ntotal, h.d, (long long)h.ntotal);
			read_flat_body(r, hs, rows);
			uint64_t nids = 0;
			r.one(nids, "the size of id_map");
			if (nids != (uint64_t)h.ntotal)
				throw_faiss(FN_READ, "faiss/impl/index_read.cpp", "id_map holds %llu ids where ntotal = %lld", (unsigned long long)nids, (long long)h.ntotal);
			ids.resize((size_t)nids);
			r.bytes(ids.data(), ids.size() * sizeof(int64_t), "id_map");
		} else if (cc == bin_fourcc("IBxF")) {
			read_header(r, h);
			read_flat_body(r, h, rows);
		} else {
			throw_faiss(FN_READ, "faiss/impl/index_read.cpp",
			            "Index type 0x%08x (\"%s\") is not a binary index this path reads (\"IBxF\", \"IBMp\", \"IBM2\"); a float index goes through read_index",
			            cc, txt);
		}
	} catch (...) {
		fclose(f);
		throw;
	}
	fclose(f);
	std::unique_ptr<BinaryIndex> ix(new BinaryIndex(h.d, idmap, idmap2));
	ix->add(h.ntotal, rows.data(), idmap ? ids.data() : nullptr);
	ix->flush();
	MVS_HIP(hipStreamSynchronize(ix->stream));
	return ix.release();
}

} // namespace mvs

// =================================================================================================
// C ABI
// =================================================================================================
using namespace mvs;

struct mvs_binary_index {
	BinaryIndex *impl = nullptr;
	SelectorCall selcall; // selector programs: option sel_bitmap_cap_bytes, statistics sel_lowered / sel_admitted of the handle's last call
	bool owned = true;
	bool sub_view = false; // the handle mvs_binary_index_idmap_sub lends: the same rows seen as the wrapped IndexBinaryFlat
	mvs_binary_index *sub_handle = nullptr;
	std::mutex own_mu;
	std::mutex *mu = &own_mu; // (a lent handle locks its owner's mutex: calls on one index are serialised)
	bool mapped() const {
		return impl->idmap && !sub_view;
	}
};

#define MVS_BIN_BEGIN try {
#define MVS_BIN_END                                                                                                    \
	}                                                                                                                  \
	catch (const std::exception &e) {                                                                                  \
		set_last_error(e.what());                                                                                      \
		return 1;                                                                                                      \
	}                                                                                                                  \
	catch (...) {                                                                                                      \
		set_last_error("unknown error");                                                                               \
		return 1;                                                                                                      \
	}                                                                                                                  \
	return 0;

extern "C" {

int mvs_binary_index_factory(mvs_binary_index **out, int d, const char *description) {
	MVS_BIN_BEGIN
	*out = nullptr;
	BinaryIndex *impl = binary_factory(d, description);
	auto *h = new mvs_binary_index;
	h->impl = impl;
	*out = h;
	MVS_BIN_END
}
void mvs_binary_index_free(mvs_binary_index *ix) {
	if (!ix)
		return;
	delete ix->sub_handle;
	if (ix->owned) {
		try {
			delete ix->impl;
		} catch (...) {
		}
	}
	delete ix;
}
int mvs_binary_index_d(const mvs_binary_index *ix) {
	return ix->impl->d;
}
int mvs_binary_index_code_size(const mvs_binary_index *ix) {
	return ix->impl->code_size;
}
int64_t mvs_binary_index_ntotal(const mvs_binary_index *ix) {
	return ix->impl->ntotal;
}
int mvs_binary_index_kind(const mvs_binary_index *ix) {
	return ix->mapped() ? MVS_BINARY_KIND_IDMAP : MVS_BINARY_KIND_FLAT;
}
mvs_binary_index *mvs_binary_index_idmap_sub(mvs_binary_index *ix) {
	if (!ix->mapped())
		return nullptr;
	if (!ix->sub_handle) {
		auto *s = new mvs_binary_index;
		s->impl = ix->impl, s->owned = false, s->sub_view = true, s->mu = ix->mu;
		ix->sub_handle = s;
	}
	return ix->sub_handle;
}
int mvs_binary_index_add(mvs_binary_index *ix, int64_t n, const uint8_t *x) {
	MVS_BIN_BEGIN
	std::lock_guard<std::mutex> g(*ix->mu);
	if (ix->mapped())
		throw_faiss("virtual void faiss::IndexBinaryIDMap::add(faiss::idx_t, const uint8_t*)", "faiss/IndexBinaryIDMap.cpp",
		            "add does not make sense with IndexBinaryIDMap, use add_with_ids");
	if (ix->sub_view)
		throw_faiss("mvs_binary_index_add", __FILE__, "rows reach the sub-index of an IndexBinaryIDMap through the wrapper's add_with_ids only");
	ix->impl->add(n, x, nullptr);
	MVS_BIN_END
}
int mvs_binary_index_add_with_ids(mvs_binary_index *ix, int64_t n, const uint8_t *x, const int64_t *ids) {
	MVS_BIN_BEGIN
	std::lock_guard<std::mutex> g(*ix->mu);
	if (!ix->mapped())
		throw_faiss("virtual void faiss::IndexBinary::add_with_ids(faiss::idx_t, const uint8_t*, const idx_t*)", "faiss/IndexBinary.cpp",
		            "add_with_ids not implemented for this type of index");
	ix->impl->add(n, x, ids);
	MVS_BIN_END
}
int mvs_binary_index_add_device(mvs_binary_index *ix, int64_t n, const uint8_t *d_x, const int64_t *d_ids, void *stream) {
	MVS_BIN_BEGIN
	std::lock_guard<std::mutex> g(*ix->mu);
	if (ix->sub_view)
		throw_faiss("mvs_binary_index_add_device", __FILE__, "rows reach the sub-index of an IndexBinaryIDMap through the wrapper's add_with_ids only");
	if (ix->mapped() && !d_ids)
		throw_faiss("virtual void faiss::IndexBinaryIDMap::add(faiss::idx_t, const uint8_t*)", "faiss/IndexBinaryIDMap.cpp",
		            "add does not make sense with IndexBinaryIDMap, use add_with_ids");
	if (!ix->mapped() && d_ids)
		throw_faiss("virtual void faiss::IndexBinary::add_with_ids(faiss::idx_t, const uint8_t*, const idx_t*)", "faiss/IndexBinary.cpp",
		            "add_with_ids not implemented for this type of index");
	ix->impl->add_device(n, d_x, d_ids, (hipStream_t)stream);
	MVS_BIN_END
}
int mvs_binary_index_search(mvs_binary_index *ix, int64_t n, const uint8_t *x, int64_t k, int32_t *distances, int64_t *labels,
                            const mvs_search_params *params) {
	MVS_BIN_BEGIN
	std::lock_guard<std::mutex> g(*ix->mu);
	SelectorCallScope sc(ix->selcall, params);
	ix->impl->search(n, x, k, distances, labels, params, ix->mapped());
	MVS_BIN_END
}
int mvs_binary_index_search_device(mvs_binary_index *ix, int64_t n, const uint8_t *d_x, int64_t k, int32_t *d_distances, int64_t *d_labels,
                                   const mvs_search_params *params, void *stream) {
	MVS_BIN_BEGIN
	std::lock_guard<std::mutex> g(*ix->mu);
	BinaryIndex *b = ix->impl;
	SelectorCallScope sc(ix->selcall, params);
	b->use_device();
	stream_wait(b->stream, (hipStream_t)stream);
	b->search_device(n, d_x, k, d_distances, d_labels, params, ix->mapped());
	stream_wait((hipStream_t)stream, b->stream);
	MVS_BIN_END
}
int mvs_binary_index_range_search(mvs_binary_index *ix, int64_t n, const uint8_t *x, int radius, const mvs_search_params *params,
                                  mvs_range_result **out) {
	MVS_BIN_BEGIN
	if (!out)
		throw_faiss("mvs_binary_index_range_search", __FILE__, "null argument");
	*out = nullptr;
	std::lock_guard<std::mutex> g(*ix->mu);
	std::unique_ptr<mvs_range_result> r(new mvs_range_result);
	r->res.clear(n);
	SelectorCallScope sc(ix->selcall, params);
	ix->impl->range_search(n, x, radius, params, ix->mapped(), r->res);
	*out = r.release();
	MVS_BIN_END
}
int mvs_binary_index_reset(mvs_binary_index *ix) {
	MVS_BIN_BEGIN
	std::lock_guard<std::mutex> g(*ix->mu);
	if (ix->sub_view)
		throw_faiss("mvs_binary_index_reset", __FILE__, "the sub-index of an IndexBinaryIDMap is reset through the wrapper");
	ix->impl->reset();
	MVS_BIN_END
}
int mvs_binary_index_reconstruct(mvs_binary_index *ix, int64_t key, uint8_t *recons) {
	MVS_BIN_BEGIN
	std::lock_guard<std::mutex> g(*ix->mu);
	ix->impl->reconstruct_n(key, 1, recons, ix->mapped(), true);
	MVS_BIN_END
}
int mvs_binary_index_reconstruct_n(mvs_binary_index *ix, int64_t i0, int64_t ni, uint8_t *recons) {
	MVS_BIN_BEGIN
	std::lock_guard<std::mutex> g(*ix->mu);
	ix->impl->reconstruct_n(i0, ni, recons, ix->mapped(), false);
	MVS_BIN_END
}
int mvs_binary_index_set_option(mvs_binary_index *ix, const char *key, int64_t value) {
	MVS_BIN_BEGIN
	std::lock_guard<std::mutex> g(*ix->mu);
	if (key && !strcmp(key, "sel_bitmap_cap_bytes")) { // (as mvs_index_set_option's: include/mi355_faiss.h "selector programs")
		if (value < 0)
			throw_faiss("mvs_binary_index_set_option", __FILE__, "sel_bitmap_cap_bytes = %lld: 0 (automatic) or a number of bytes", (long long)value);
		ix->selcall.cap_bytes = value;
		return 0;
	}
	if (!ix->impl->set_option(key, value))
		throw_faiss("mvs_binary_index_set_option", __FILE__, "unknown option %s", key);
	MVS_BIN_END
}
int mvs_binary_index_get_stat(mvs_binary_index *ix, const char *name, int64_t *value) {
	MVS_BIN_BEGIN
	std::lock_guard<std::mutex> g(*ix->mu);
	if (name && value && (!strcmp(name, "sel_lowered") || !strcmp(name, "sel_admitted"))) {
		*value = !strcmp(name, "sel_lowered") ? (int64_t)ix->selcall.lowered : ix->selcall.admitted;
		return 0;
	}
	if (!ix->impl->get_stat(name, value))
		throw_faiss("mvs_binary_index_get_stat", __FILE__, "unknown statistic %s", name);
	MVS_BIN_END
}
int mvs_write_index_binary(mvs_binary_index *ix, const char *filename) {
	MVS_BIN_BEGIN
	std::lock_guard<std::mutex> g(*ix->mu);
	if (ix->sub_view)
		throw_faiss("mvs_write_index_binary", __FILE__, "the sub-index of an IndexBinaryIDMap is written with its wrapper");
	write_binary_file(ix->impl, filename);
	MVS_BIN_END
}
int mvs_read_index_binary(mvs_binary_index **out, const char *filename) {
	MVS_BIN_BEGIN
	*out = nullptr;
	BinaryIndex *impl = read_binary_file(filename);
	auto *h = new mvs_binary_index;
	h->impl = impl;
	*out = h;
	MVS_BIN_END
}

} // extern "C"
