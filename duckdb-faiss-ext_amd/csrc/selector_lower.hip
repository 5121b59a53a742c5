// csrc/selector_lower.hip -- MVS_SEL_PROGRAM on the device (include/mi355_faiss.h "selector programs"): the program is
// evaluated once per call over the ids the call's scan will test (the IdDomain) and lowered to one of the two plain selectors every scan
// kernel already understands.  No scan kernel knows programs.
//
//   selector_eval_kernel     one domain entry per lane: the packed program (csrc/selector_program.h) walked with a 64-bit stack of bits; one
//                            admitted bit per entry (a wave ballot = one 64-bit word), and (count, min, max) of the admitted ids
//   selector_scatter_kernel  bitmap lowering: bit `id` of the zeroed buffer, 32-bit atomicOr
//   selector_compact_kernel  batch lowering: the admitted ids in any order (one atomicAdd per wave word); rocprim sorts them afterwards
#include "index.h"
#include "selector_program.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <chrono>
#include <cstdlib>

namespace mvs {

thread_local SelectorCall *t_selector_call = nullptr;

namespace {

constexpr unsigned SEL_MAX_BLOCKS = 4096; // (grid-stride loops)
constexpr unsigned long long SIGN64 = 0x8000000000000000ull; // id ^ SIGN64 orders signed ids as unsigned

struct SelLowerStats {
	unsigned long long count, min_biased, max_biased, cursor; // cursor: selector_compact_kernel's fill
};

// entry i of an IdDomain (csrc/index.h)
__device__ __forceinline__ long long domain_id(const long long *__restrict__ ids, long long off, const long long *__restrict__ map, long long i) {
	const long long raw = ids ? ids[i] : off + i;
	return map ? map[raw] : raw;
}

__device__ __forceinline__ bool lower_leaf_member(const SelPackedNode &p, const uint8_t *__restrict__ blob, long long id) {
	if (p.op == MVS_SELOP_ALL)
		return true;
	if (p.op == MVS_SELOP_RANGE)
		return id >= p.imin && id < p.imax;
	if (p.op == MVS_SELOP_BITMAP) {
		const unsigned long long u = (unsigned long long)id;
		if ((u >> 3) >= (unsigned long long)p.n)
			return false;
		return (blob[p.off + (long long)(u >> 3)] >> (u & 7)) & 1;
	}
	const long long *ids = (const long long *)(blob + p.off); // (offsets are multiples of 8)
	long long lo = 0, hi = p.n;
	while (lo < hi) {
		const long long mid = (lo + hi) >> 1;
		if (ids[mid] < id)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo < p.n && ids[lo] == id;
}

// the program is the same for every lane: the op dispatch is uniform control flow, only the leaves' data differ per lane
__device__ __forceinline__ bool lower_member(const SelPackedNode *__restrict__ nodes, int nn, const uint8_t *__restrict__ blob, long long id) {
	unsigned long long stk = 0; // bit 0 is the top
	for (int i = 0; i < nn; ++i) {
		const SelPackedNode p = nodes[i];
		if (p.op == MVS_SELOP_NOT) {
			stk ^= 1ull;
		} else if (p.op == MVS_SELOP_AND || p.op == MVS_SELOP_OR || p.op == MVS_SELOP_XOR) {
			const unsigned long long b = stk & 1ull;
			stk >>= 1;
			const unsigned long long a = stk & 1ull;
			const unsigned long long r = p.op == MVS_SELOP_AND ? (a & b) : p.op == MVS_SELOP_OR ? (a | b) : (a ^ b);
			stk = (stk & ~1ull) | r;
		} else {
			stk = (stk << 1) | (lower_leaf_member(p, blob, id) ? 1ull : 0ull);
		}
	}
	return stk & 1ull;
}

// bits [ceil(n / 64)]: bit (i & 63) of word i >> 6 says entry i is admitted.  Every lane of a wave runs every iteration (the ballot needs them
// all); a lane past n votes 0, and a wave whose 64 entries all lie past n writes nothing
__global__ __launch_bounds__(256) void selector_eval_kernel(const SelPackedNode *__restrict__ nodes, int nn, const uint8_t *__restrict__ blob,
                                                            const long long *__restrict__ ids, long long off, const long long *__restrict__ map,
                                                            long long n, unsigned long long *__restrict__ bits, SelLowerStats *__restrict__ stats) {
	unsigned long long cnt = 0, mn = ~0ull, mx = 0;
	const long long nround = (n + 255) & ~255ll;
	for (long long base = (long long)blockIdx.x * 256; base < nround; base += (long long)gridDim.x * 256) {
		const long long i = base + threadIdx.x;
		bool adm = false;
		if (i < n) {
			const long long id = domain_id(ids, off, map, i);
			adm = lower_member(nodes, nn, blob, id);
			if (adm) {
				const unsigned long long u = (unsigned long long)id ^ SIGN64;
				++cnt;
				mn = u < mn ? u : mn;
				mx = u > mx ? u : mx;
			}
		}
		const unsigned long long word = __ballot(adm);
		const long long wbase = base + (threadIdx.x & ~63u);
		if ((threadIdx.x & 63u) == 0 && wbase < n)
			bits[wbase >> 6] = word;
	}
	for (int o = 32; o > 0; o >>= 1) {
		cnt += __shfl_xor(cnt, o);
		const unsigned long long omn = __shfl_xor(mn, o), omx = __shfl_xor(mx, o);
		mn = omn < mn ? omn : mn;
		mx = omx > mx ? omx : mx;
	}
	__shared__ unsigned long long s_cnt[4], s_mn[4], s_mx[4];
	if ((threadIdx.x & 63u) == 0) {
		s_cnt[threadIdx.x >> 6] = cnt;
		s_mn[threadIdx.x >> 6] = mn;
		s_mx[threadIdx.x >> 6] = mx;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < 4; ++w) {
			cnt += s_cnt[w];
			mn = s_mn[w] < mn ? s_mn[w] : mn;
			mx = s_mx[w] > mx ? s_mx[w] : mx;
		}
		if (cnt) {
			atomicAdd(&stats->count, cnt);
			atomicMin(&stats->min_biased, mn);
			atomicMax(&stats->max_biased, mx);
		}
	}
}

// every admitted id is >= 0 and id >> 3 < nbytes (the lowering rule checked min and max); words [ceil(nbytes / 4)] are zero on entry
__global__ __launch_bounds__(256) void selector_scatter_kernel(const unsigned long long *__restrict__ bits, const long long *__restrict__ ids, long long off,
                                                               const long long *__restrict__ map, long long n, unsigned *__restrict__ words) {
	for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
		if (!((bits[i >> 6] >> (i & 63)) & 1ull))
			continue;
		const unsigned long long id = (unsigned long long)domain_id(ids, off, map, i);
		atomicOr(words + (id >> 5), 1u << (id & 31));
	}
}

// out [count]: the admitted ids, unordered.  A wave takes its 64 entries' places with one atomicAdd
__global__ __launch_bounds__(256) void selector_compact_kernel(const unsigned long long *__restrict__ bits, const long long *__restrict__ ids, long long off,
                                                               const long long *__restrict__ map, long long n, long long cap, long long *__restrict__ out, SelLowerStats *__restrict__ stats) {
	const long long nround = (n + 255) & ~255ll;
	const unsigned lane = threadIdx.x & 63u;
	for (long long base = (long long)blockIdx.x * 256; base < nround; base += (long long)gridDim.x * 256) {
		const long long i = base + threadIdx.x;
		const long long wbase = base + (threadIdx.x & ~63u);
		if (wbase >= n) // (the whole wave)
			continue;
		const unsigned long long word = bits[wbase >> 6];
		if (!word)
			continue;
		unsigned long long first = 0;
		if (lane == 0)
			first = atomicAdd(&stats->cursor, (unsigned long long)__popcll(word));
		first = __shfl(first, 0);
		if ((word >> lane) & 1ull) {
			const long long dst = (long long)first + __popcll(word & ((1ull << lane) - 1ull));
			if (dst < cap) // (word bits past n are 0, and count entries were reserved: always true)
				out[dst] = domain_id(ids, off, map, i);
		}
	}
}

unsigned lower_grid(long long n) {
	return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, (long long)SEL_MAX_BLOCKS));
}

} // namespace

SelectorCallScope::SelectorCallScope(SelectorCall &c, const mvs_search_params *p) : prev(t_selector_call) {
	if (p && p->sel_kind == MVS_SEL_PROGRAM) {
		const std::string err = sel_program_validate((const mvs_sel_node *)p->sel_data, p->sel_n);
		if (!err.empty())
			throw_faiss("faiss::IDSelector", __FILE__, "selector program: %s", err.c_str());
	}
	c.lowered = 0, c.admitted = 0;
	t_selector_call = &c;
}
SelectorCallScope::~SelectorCallScope() {
	t_selector_call = prev;
}

void SelectorHolder::release() {
	buf.release(), prog.release(), bits.release(), ids.release(), temp.release(), stats.release();
}

SelectorDev SelectorHolder::upload_program(const mvs_search_params *p, const IdDomain &dom, hipStream_t st) {
	const mvs_sel_node *nodes = (const mvs_sel_node *)p->sel_data;
	const std::string err = sel_program_validate(nodes, p->sel_n);
	if (!err.empty())
		throw_faiss("faiss::IDSelector", __FILE__, "selector program: %s", err.c_str());
	// one leaf that IS a plain selector: today's path, unchanged (no evaluation, no synchronisation)
	if (p->sel_n == 1 && (nodes[0].op == MVS_SELOP_BITMAP || nodes[0].op == MVS_SELOP_BATCH || nodes[0].op == MVS_SELOP_ARRAY)) {
		mvs_search_params q = *p;
		q.sel_kind = nodes[0].op == MVS_SELOP_BITMAP ? MVS_SEL_BITMAP : MVS_SEL_BATCH;
		q.sel_data = nodes[0].data;
		q.sel_n = nodes[0].n;
		return upload(&q, dom, st);
	}
	SelectorDev s;
	memset(&s, 0, sizeof s);
	SelectorCall *call = t_selector_call;
	const int64_t n = std::max<int64_t>(dom.n, 0);
	// (MVS_SELECTOR_PROFILE=1: what the lowering costs, on stderr, the stream synchronised before and after -- tools/selector_bench.py)
	struct Profile {
		const bool on = getenv("MVS_SELECTOR_PROFILE") != nullptr;
		hipStream_t st;
		int64_t n;
		const SelectorDev &s;
		std::chrono::steady_clock::time_point t0;
		Profile(hipStream_t st_, int64_t n_, const SelectorDev &s_) : st(st_), n(n_), s(s_) {
			if (on) {
				(void)hipStreamSynchronize(st);
				t0 = std::chrono::steady_clock::now();
			}
		}
		~Profile() {
			if (!on)
				return;
			(void)hipStreamSynchronize(st);
			fprintf(stderr, "selprofile\tlowering of %lld ids to %s: %.3f ms\n", (long long)n, s.kind == MVS_SEL_BITMAP ? "a bitmap" : "a batch",
			        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
		}
	} profile(st, n, s);
	SelLowerStats hs = {0, ~0ull, 0, 0};
	if (n > 0) {
		SelProgram pk;
		sel_program_pack(nodes, p->sel_n, pk);
		const size_t node_bytes = pk.nodes.size() * sizeof(SelPackedNode);
		prog.reserve(node_bytes + std::max<size_t>(pk.blob.size(), 8));
		bits.reserve((size_t)((n + 63) / 64) * sizeof(unsigned long long));
		stats.reserve(sizeof(SelLowerStats));
		// (pageable host memory: each copy has left `pk` / `hs` when the call returns)
		MVS_HIP(hipMemcpyAsync(prog.p, pk.nodes.data(), node_bytes, hipMemcpyHostToDevice, st));
		if (!pk.blob.empty())
			MVS_HIP(hipMemcpyAsync((char *)prog.p + node_bytes, pk.blob.data(), pk.blob.size(), hipMemcpyHostToDevice, st));
		MVS_HIP(hipMemcpyAsync(stats.p, &hs, sizeof hs, hipMemcpyHostToDevice, st));
		hipLaunchKernelGGL(selector_eval_kernel, dim3(lower_grid(n)), dim3(256), 0, st, (const SelPackedNode *)prog.p, (int)pk.nodes.size(),
		                   (const uint8_t *)prog.p + node_bytes, (const long long *)dom.d_ids, (long long)dom.offset, (const long long *)dom.d_map,
		                   (long long)n, (unsigned long long *)bits.p, (SelLowerStats *)stats.p);
		MVS_HIP(hipGetLastError());
		// the one readback of the lowering: (count, min, max) decide the form.  A synchronisation point (MVS_SEL_BATCH sorts on the host instead)
		MVS_HIP(hipMemcpyAsync(&hs, stats.p, sizeof hs, hipMemcpyDeviceToHost, st));
		MVS_HIP(hipStreamSynchronize(st));
	}
	const int64_t count = (int64_t)hs.count;
	if (call)
		call->admitted = count;
	if (count == 0) { // (also the empty index: nothing was launched)
		buf.reserve(8);
		s.kind = MVS_SEL_BATCH;
		s.sorted_ids = (const int64_t *)buf.p;
		s.nids = 0;
		if (call)
			call->lowered = 2;
		return s;
	}
	const int64_t mn = (int64_t)(hs.min_biased ^ SIGN64), mx = (int64_t)(hs.max_biased ^ SIGN64);
	// the cap: a bitmap costs max / 8 bytes whatever the count, a batch 8 bytes per admitted id and a bisection per tested row; 2 bytes per
	// tested id (16 id values per entry) keeps the bitmap below the batch it replaces unless fewer than a quarter are admitted, and 1 MiB is
	// always affordable
	int64_t cap = call ? call->cap_bytes : 0;
	if (cap <= 0)
		cap = std::max<int64_t>((int64_t)1 << 20, 2 * n);
	if (mn >= 0 && (mx >> 3) + 1 <= cap) {
		const int64_t nbytes = (mx >> 3) + 1;
		const size_t padded = (size_t)((nbytes + 3) & ~(int64_t)3);
		buf.reserve(padded);
		MVS_HIP(hipMemsetAsync(buf.p, 0, padded, st));
		hipLaunchKernelGGL(selector_scatter_kernel, dim3(lower_grid(n)), dim3(256), 0, st, (const unsigned long long *)bits.p, (const long long *)dom.d_ids,
		                   (long long)dom.offset, (const long long *)dom.d_map, (long long)n, (unsigned *)buf.p);
		MVS_HIP(hipGetLastError());
		s.kind = MVS_SEL_BITMAP;
		s.bitmap = (const uint8_t *)buf.p;
		s.nbytes = nbytes;
		if (call)
			call->lowered = 1;
		return s;
	}
	ids.reserve((size_t)count * sizeof(int64_t));
	buf.reserve((size_t)count * sizeof(int64_t));
	hipLaunchKernelGGL(selector_compact_kernel, dim3(lower_grid(n)), dim3(256), 0, st, (const unsigned long long *)bits.p, (const long long *)dom.d_ids,
	                   (long long)dom.offset, (const long long *)dom.d_map, (long long)n, (long long)count, (long long *)ids.p, (SelLowerStats *)stats.p);
	MVS_HIP(hipGetLastError());
	size_t tb = 0;
	MVS_HIP(rocprim::radix_sort_keys(nullptr, tb, (const long long *)ids.p, (long long *)buf.p, (size_t)count, 0, 64, st));
	temp.reserve(std::max<size_t>(tb, 16));
	MVS_HIP(rocprim::radix_sort_keys(temp.p, tb, (const long long *)ids.p, (long long *)buf.p, (size_t)count, 0, 64, st));
	s.kind = MVS_SEL_BATCH;
	s.sorted_ids = (const int64_t *)buf.p;
	s.nids = count;
	if (call)
		call->lowered = 2;
	return s;
}

} // namespace mvs
