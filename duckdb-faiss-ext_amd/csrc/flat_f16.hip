// csrc/flat_f16.hip -- half-precision Flat (MVS_KIND_FLAT16): what faiss-gpu's GpuClonerOptions::useFloat16 gives a Flat index.  The rows
// are IEEE fp16, the scores come from v_mfma_f32_16x16x32_f16 and ARE the answer: no re-scoring pass.  The contract is the "half-precision
// Flat" section of include/mi355_faiss.h; the design and the measurements are DESIGN.md 3.19.  An index of this kind is made by
// mvs_index_clone_to_gpu_opts from a Flat index (or IDMap / IDMap2 over one); FlatIndex, its stores and its kernels are not involved.
//
// Store.  Fragment-major fp16: the 8 halves one lane feeds one 16x16x32 MFMA k-step are ONE aligned 16-byte word.  Word
//   ((row >> 4) S + (k >> 5)) 64 + ((k & 31) >> 3) 16 + (row & 15)          S = dpad / 32 k-steps, dpad = d rounded up to 32
// holds components k & ~7 .. of `row`, so the 64 words of (16 rows, one k-step) are 1 KB in lane order: a wave's operand load is one
// coalesced 16-byte-per-lane access and nothing is permuted on the way to the matrix pipe.  Rows are padded to whole 64-row tiles and d to
// 32, both with zeros; n_i (one f32 per row) is the fmaf chain over the decoded halves, k ascending from +0, computed once at add time
// (this translation unit is compiled with contraction off, as csrc/sq.hip).  The arrival-order [n][d] view is derived from the word
// formula (RECON_F16 in csrc/reconstruct.hip): no second copy.  Growth is append-only (DevMem::regrow: zeroed, the prefix kept).
//
// Scan (flat16_scan_reg_kernel<S>, d <= 128; flat16_scan_lds_kernel, d > 128).  Operand A = 16 database rows, operand B = 16 queries: lane l
// of the result holds rows 4 (l >> 4) .. + 3 of the 16 for query l & 15, so a lane tests FOUR rows against ONE query's bound.
//   work split   a workgroup is 4 waves (one per SIMD).  blockIdx.x picks the query block, blockIdx.y the row lane; a wave walks 64-row
//                tiles (4 x 16 rows) tile0 + y, + gridDim.y ...  d <= 128: a wave OWNS 64 queries whose fragments stay in registers for
//                the whole launch; with nq > 64 the 4 waves of a workgroup take 4 different query groups and the SAME tiles, so a tile
//                is fetched from L2 once and three times from the CU's L1.  d > 128: the workgroup's 32 queries sit in LDS in fragment
//                order, the 4 waves take different tiles and walk the k-steps, two ds_read_b128 per k-step per lane.
//   LDS          d <= 128: none.  d > 128: S x 2 KB (query fragments), 10 KB at d = 160, 128 KB of the CU's 160 KB at d = 2048.
//   registers    d = 128: 64 VGPRs of query fragments (4 groups x 4 steps x 4), 64 of row fragments, 16 accumulators (one 16-row
//                operand against the 4 query groups at a time), 16 of bounds and norms: 232 as compiled, two waves per SIMD, no spill.
//                d > 128: 32 accumulators, 16 of row fragments, 8 of query fragments: 122 as compiled.
//   pace         per 64-row tile a wave issues 16 S MFMAs and tests 64 (d <= 128) or 32 scores per lane on the vector ALU (the L2 form,
//                the clamp, one compare per score, one ballot per four).  The row fragments come straight from global memory into
//                registers (1 KB per load, no LDS round trip); nothing is prefetched by hand: the other wave of the SIMD is what covers
//                a tile's loads.  Measured at N = 10 M, d = 128, nq = 10 k: the scan runs at 18 - 20 % of the f16 matrix peak.  By
//                instruction count the tests outweigh the matrix work (64 MFMAs a tile against 256 scores a lane); which unit the loop
//                waits for has not been measured with counters (DESIGN.md 3.19 has the table).
//
// Selection, as csrc/binary.hip: no k-lists in the scan.  A row is admitted iff it passes the admission rule of csrc/pq_kernels.h (no
// NaN, strictly better than +-FLT_MAX) and its PAIR (order key of the score, row) is below the query's bound T(q), the exact k-th pair of
// all rows scanned in earlier generations; admitted pairs go to a record stream, rows are scanned in generations of geometrically growing
// ranges and flat16_select_kernel merges a query's records after each.  The pair order is total, so results depend neither on generation
// sizes nor on the stream's capacity nor on the order of the atomics.  A selector becomes one allowed-bit per row (flat16_allow_kernel):
// the scan has one masked path.
//
// Refused with "This index type is not implemented on the MI355X path yet: ...": range_search, remove_ids, merge_from /
// check_compatible_for_merge, search_and_reconstruct, sharding and clone_to_gpu(-1), another device (to_gpu), metrics beyond L2 / inner
// product, d > 2048, k > 2048.
#include "flat16_select.h"

#include <rocprim/device/device_scan.hpp>

#include <cstring>
#include <memory>

#pragma clang fp contract(off)

namespace mvs {

namespace {

const char *const FN_NOT_IMPL = "faiss::Index* faiss::gpu::index_cpu_to_gpu(...)";
// (the constants, the score test, the record stream and the generation kernels are in csrc/flat16_select.h, shared with csrc/bf_knn.hip)

// ---------------------------------------------------------------------------------------------- add path: convert + pack, norms
// Rows [row0, row0 + n) of the store from x [n][d] f32 (round to nearest even: v_cvt_f16_f32 -- overflow to +-inf, subnormals kept, NaN
// stays NaN).  One thread per 16-byte word of the 16-row groups [row0 >> 4, gend): rows below row0 keep their words, rows at and beyond
// row0 + n (the tile's padding, or what a reset left behind) become zeros
__global__ __launch_bounds__(256) void flat16_pack_kernel(const float *__restrict__ x, long long n, int d, int S, long long row0, long long gend,
                                                          uint4 *__restrict__ words) {
	const long long g0 = row0 >> 4, total = (gend - g0) * S * 64;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const int lane = (int)(i & 63);
		const long long gs = i >> 6;
		const long long grp = g0 + gs / S;
		const int s = (int)(gs % S);
		const long long row = grp * 16 + (lane & 15);
		if (row < row0)
			continue;
		const int k0 = 32 * s + 8 * (lane >> 4);
		unsigned h[8];
#pragma unroll
		for (int e = 0; e < 8; ++e) {
			float v = 0.f;
			if (row < row0 + n && k0 + e < d)
				v = x[(row - row0) * d + k0 + e];
			h[e] = (unsigned)__half_as_ushort(__float2half_rn(v));
		}
		words[(grp * S + s) * 64 + lane] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
	}
}


// ---------------------------------------------------------------------------------------------- selector: one allowed-bit per row
// allow[t] bit b = row 64 t + b exists and its id (ids[row], or the row number) is a member
__global__ __launch_bounds__(256) void flat16_allow_kernel(SelectorDev sel, const long long *__restrict__ ids, long long n, long long ntiles,
                                                           unsigned long long *__restrict__ allow) {
	const int lane = threadIdx.x & 63;
	for (long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); tile < ntiles; tile += (long long)gridDim.x * 4) {
		const long long row = tile * 64 + lane;
		bool ok = false;
		if (row < n)
			ok = pq_sel_member(sel, ids ? ids[row] : row);
		const unsigned long long m = __ballot(ok);
		if (lane == 0)
			allow[tile] = m;
	}
}


// d <= 128: S k-steps, the wave's 64 queries resident in registers
template <int S>
__global__ __launch_bounds__(256, 2) void flat16_scan_reg_kernel(const F16Scan a) {
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
	const int qwave = w % a.nqw, rl = w / a.nqw, nrl = 4 / a.nqw;
	const int q0 = (blockIdx.x * a.nqw + qwave) * 64;
	if (q0 >= a.nq)
		return; // (uniform over the wave; the kernel has no barrier)
	f16x8 qf[4][S];
	F16Bound bd[4];
#pragma unroll
	for (int j = 0; j < 4; ++j) {
#pragma unroll
		for (int s = 0; s < S; ++s)
			qf[j][s] = *reinterpret_cast<const f16x8 *>(a.qf + ((size_t)((q0 >> 4) + j) * S + s) * 64 + lane);
		bd[j] = f16_bound(a, q0 + 16 * j + col);
	}
	for (long long tile = a.tile0 + (long long)blockIdx.y * nrl + rl; tile < a.tile1; tile += (long long)gridDim.y * nrl) {
		const uint4 *tp = a.rows + (size_t)tile * 4 * S * 64 + lane;
		f16x8 af[4][S];
#pragma unroll
		for (int i = 0; i < 4; ++i)
#pragma unroll
			for (int s = 0; s < S; ++s)
				af[i][s] = *reinterpret_cast<const f16x8 *>(tp + (i * S + s) * 64);
		const unsigned long long aw = a.allow ? a.allow[tile] : ~0ull;
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			f32x4 acc[4];
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				acc[j] = f32x4 {0.f, 0.f, 0.f, 0.f};
#pragma unroll
				for (int s = 0; s < S; ++s)
					acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][s], qf[j][s], acc[j], 0, 0, 0);
			}
			const long long row4 = tile * 64 + 16 * i + 4 * g;
			const float4 nr = *reinterpret_cast<const float4 *>(a.norms + row4);
#pragma unroll
			for (int j = 0; j < 4; ++j)
				f16_test4(a, acc[j], bd[j], nr, row4, q0 + 16 * j + col, aw, 16 * i + 4 * g, lane);
		}
	}
}

// d > 128: the workgroup's 32 queries in LDS as [S][2][64] words, the 4 waves on different tiles, the k-steps walked
__global__ __launch_bounds__(256, 2) void flat16_scan_lds_kernel(const F16Scan a) {
	extern __shared__ __attribute__((aligned(16))) uint4 f16_lds[];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
	const int q0 = blockIdx.x * 32, S = a.S;
	for (int i = threadIdx.x; i < S * 128; i += 256) {
		const int s = i >> 7, j = (i >> 6) & 1, ln = i & 63;
		f16_lds[i] = a.qf[((size_t)((q0 >> 4) + j) * S + s) * 64 + ln];
	}
	__syncthreads();
	F16Bound bd[2];
#pragma unroll
	for (int j = 0; j < 2; ++j)
		bd[j] = f16_bound(a, q0 + 16 * j + col);
	for (long long tile = a.tile0 + (long long)blockIdx.y * 4 + w; tile < a.tile1; tile += (long long)gridDim.y * 4) {
		const uint4 *tp = a.rows + (size_t)tile * 4 * S * 64 + lane;
		f32x4 acc[4][2];
#pragma unroll
		for (int i = 0; i < 4; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				acc[i][j] = f32x4 {0.f, 0.f, 0.f, 0.f};
		for (int s = 0; s < S; ++s) {
			const f16x8 b0 = *reinterpret_cast<const f16x8 *>(f16_lds + (s * 2 + 0) * 64 + lane);
			const f16x8 b1 = *reinterpret_cast<const f16x8 *>(f16_lds + (s * 2 + 1) * 64 + lane);
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				const f16x8 av = *reinterpret_cast<const f16x8 *>(tp + ((size_t)i * S + s) * 64);
				acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, b0, acc[i][0], 0, 0, 0);
				acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, b1, acc[i][1], 0, 0, 0);
			}
		}
		const unsigned long long aw = a.allow ? a.allow[tile] : ~0ull;
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const long long row4 = tile * 64 + 16 * i + 4 * g;
			const float4 nr = *reinterpret_cast<const float4 *>(a.norms + row4);
#pragma unroll
			for (int j = 0; j < 2; ++j)
				f16_test4(a, acc[i][j], bd[j], nr, row4, q0 + 16 * j + col, aw, 16 * i + 4 * g, lane);
		}
	}
}


// diagnostics: ONE v_mfma_f32_16x16x32_f16 per wavefront on caller-supplied tiles, the twin of mfma_bf16_probe_kernel (csrc/util_kernels.hip).
// A: [ntiles][16 rows][32 k] fp16 bits, Bt: [ntiles][16 columns][32 k] fp16 bits, C / D: [ntiles][16 rows][16 columns] f32
__global__ __launch_bounds__(64) void mfma_f16_probe_kernel(const unsigned short *__restrict__ A, const unsigned short *__restrict__ Bt,
                                                            const float *__restrict__ C, float *__restrict__ D) {
	const size_t t = blockIdx.x;
	const int l = threadIdx.x, rc = l & 15, g = l >> 4;
	const f16x8 av = *reinterpret_cast<const f16x8 *>(A + t * 512 + rc * 32 + 8 * g);  // row rc, k = 8 g .. 8 g + 7
	const f16x8 bv = *reinterpret_cast<const f16x8 *>(Bt + t * 512 + rc * 32 + 8 * g); // column rc, the same k
	f32x4 c;
#pragma unroll
	for (int r = 0; r < 4; ++r)
		c[r] = C[t * 256 + (4 * g + r) * 16 + rc];
	const f32x4 dv = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, c, 0, 0, 0);
#pragma unroll
	for (int r = 0; r < 4; ++r)
		D[t * 256 + (4 * g + r) * 16 + rc] = dv[r];
}

[[noreturn]] void f16_refuse(const char *what) {
	throw_faiss(FN_NOT_IMPL, "faiss/gpu/GpuCloner.cpp", "This index type is not implemented on the MI355X path yet: %s", what);
}

// ---------------------------------------------------------------------------------------------- the index
class Flat16Index : public IndexBase {
public:
	const int S; // k-steps of 32 per row

	Flat16Index(int d_, int metric_) : IndexBase(MVS_KIND_FLAT16, d_, metric_), S((d_ + 31) / 32) {
	}

	void reset() {
		use_device();
		MVS_HIP(hipStreamSynchronize(stream));
		ntotal = 0; // (the next add rewrites its tile from its first row on: flat16_pack_kernel zeroes what follows)
	}
	size_t device_bytes() const override {
		return words_.cap + norms_.cap;
	}
	// room for `rows` rows in whole tiles: exactly, where the store is empty (a clone knows its size), else by half again
	void reserve_rows(int64_t rows) {
		const int64_t need = (rows + F16_TILE - 1) / F16_TILE * F16_TILE;
		if (need <= cap)
			return;
		if (need > ((int64_t)1 << 31) - 1024)
			throw_faiss("mvs::Flat16Index::add", __FILE__, "%lld rows are beyond the 2^31 - 1024 rows a half-precision Flat index holds", (long long)rows);
		const int64_t ncap = cap == 0 ? need : std::max(need, (cap + cap / 2 + F16_TILE - 1) / F16_TILE * F16_TILE);
		const int64_t used = (ntotal + F16_TILE - 1) / F16_TILE * F16_TILE;
		try {
			words_.regrow((size_t)ncap * S * 64, (size_t)used * S * 64, true, stream); // (rows / 16 groups x S x 64 words x 16 bytes)
			norms_.regrow((size_t)ncap * sizeof(float), (size_t)used * sizeof(float), true, stream);
		} catch (...) {
			throw_faiss("mvs::Flat16Index::grow", __FILE__, "out of device memory for %lld rows of %d halves", (long long)ncap, 32 * S);
		}
		cap = ncap;
	}

	// ---- add: rows [ntotal, ntotal + n) from device f32 rows, on the index's stream: convert + pack, then the norms
	void append_device(int64_t n, const float *d_x) {
		reserve_rows(ntotal + n);
		const int64_t gend = (ntotal + n + F16_TILE - 1) / F16_TILE * (F16_TILE / 16);
		hipLaunchKernelGGL(flat16_pack_kernel, dim3(grid_for((gend - (ntotal >> 4)) * S * 64)), dim3(256), 0, stream, d_x, (long long)n, d, S,
		                   (long long)ntotal, (long long)gend, (uint4 *)words_.p);
		hipLaunchKernelGGL(flat16_norm_kernel, dim3(grid_for(n)), dim3(256), 0, stream, (const uint4 *)words_.p, S, (long long)ntotal, (long long)n,
		                   (float *)norms_.p + ntotal);
		const int64_t pad = gend * 16 - (ntotal + n); // (the norms of the tile's padding: zero, also after a reset)
		if (pad > 0)
			MVS_HIP(hipMemsetAsync((float *)norms_.p + ntotal + n, 0, (size_t)pad * sizeof(float), stream));
		MVS_HIP(hipGetLastError());
		ntotal += n;
	}
	void add(int64_t n, const float *x) override {
		use_device();
		const int64_t chunk = std::max<int64_t>(1, (int64_t)PinnedRing::SLOT_BYTES / ((int64_t)d * 4));
		for (int64_t i0 = 0; i0 < n; i0 += chunk) {
			const int64_t nc = std::min(chunk, n - i0);
			const size_t bytes = (size_t)nc * d * sizeof(float);
			ws_add.reserve(bytes);
			const int slot = pinned.acquire(bytes);
			memcpy(pinned.buf[slot], x + i0 * d, bytes);
			MVS_HIP(hipMemcpyAsync(ws_add.p, pinned.buf[slot], bytes, hipMemcpyHostToDevice, stream));
			pinned.release(slot, stream);
			append_device(nc, (const float *)ws_add.p);
		}
	}
	void add_device(int64_t n, const float *d_x, hipStream_t st) override {
		use_device();
		if (n <= 0)
			return;
		stream_wait(stream, st);
		append_device(n, d_x);
		stream_wait(st, stream);
	}

	// ---- search
	void search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, hipStream_t st) override {
		search_mapped(nq, d_x, k, d_D, d_I, params, nullptr, st);
	}
	void search_mapped(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, const int64_t *d_idmap,
	                   hipStream_t st) override {
		use_device();
		if (k <= 0)
			throw_faiss("virtual void faiss::Index::search(...) const", "faiss/Index.cpp", "Error: 'k > 0' failed");
		if (k > F16_MAX_K) {
			char what[96];
			snprintf(what, sizeof what, "half-precision Flat with k = %lld (at most %d)", (long long)k, F16_MAX_K);
			f16_refuse(what);
		}
		if (nq <= 0)
			return;
		stream_wait(st, stream); // (adds were enqueued on the index's stream)
		scan_launches = 0, candidates = 0;
		const int desc = metric == METRIC_L2 ? 0 : 1;
		const long long *map = (const long long *)d_idmap;
		const int64_t n = ntotal, ntiles = (n + F16_TILE - 1) / F16_TILE;
		if (n == 0) {
			hipLaunchKernelGGL(flat16_emit_kernel, dim3(grid_for(nq * k)), dim3(256), 0, st, (const unsigned long long *)nullptr, (long long)(nq * k), desc,
			                   map, (long long)label_offset, d_D, (long long *)d_I);
			MVS_HIP(hipGetLastError());
			return;
		}
		const unsigned long long *allow = nullptr;
		if (params && params->sel_kind != MVS_SEL_NONE) {
			const SelectorDev sel = selector.upload(params, IdDomain::rows(0, n, d_idmap), st); // (the mask tests map[row], or the row)
			ws_allow.reserve((size_t)ntiles * 8);
			hipLaunchKernelGGL(flat16_allow_kernel, dim3(grid_for(ntiles, 4)), dim3(256), 0, st, sel, map, (long long)n, (long long)ntiles,
			                   (unsigned long long *)ws_allow.p);
			MVS_HIP(hipGetLastError());
			allow = (const unsigned long long *)ws_allow.p;
		}
		int K2 = 256;
		while (K2 < k)
			K2 <<= 1;
		// rows examined before the first bound exists: at least k of them, whole tiles
		const int64_t first = (std::max<int64_t>(first_rows, k) + F16_TILE - 1) / F16_TILE * F16_TILE;
		int generations = 0, grid_last = 0;
		for (int64_t q0 = 0; q0 < nq; q0 += F16_QCHUNK) {
			const int64_t nc = std::min(F16_QCHUNK, nq - q0), ncp = (nc + 63) / 64 * 64;
			ws_q.reserve((size_t)ncp * S * 64);
			ws_qn.reserve((size_t)ncp * sizeof(float));
			ws_best.reserve((size_t)nc * k * 8);
			ws_ctl.reserve(64 + (size_t)ncp * 8 + 3 * (size_t)(nc + 1) * 4 + 64);
			unsigned long long *d_cnt = (unsigned long long *)ws_ctl.p;
			unsigned long long *d_T = (unsigned long long *)((char *)ws_ctl.p + 64);
			unsigned *d_qcnt = (unsigned *)(d_T + ncp), *d_qoff = d_qcnt + (nc + 1), *d_qfill = d_qoff + (nc + 1);
			// the queries as the rows are: rounded to fp16, packed, m_q by the same chain
			hipLaunchKernelGGL(flat16_pack_kernel, dim3(grid_for(ncp / 16 * S * 64)), dim3(256), 0, st, d_x + (size_t)q0 * d, (long long)nc, d, S, 0ll,
			                   (long long)(ncp / 16), (uint4 *)ws_q.p);
			hipLaunchKernelGGL(flat16_norm_kernel, dim3(grid_for(ncp)), dim3(256), 0, st, (const uint4 *)ws_q.p, S, 0ll, (long long)ncp, (float *)ws_qn.p);
			hipLaunchKernelGGL(flat16_fill_kernel, dim3(grid_for(nc * k)), dim3(256), 0, st, (unsigned long long *)ws_best.p, (long long)(nc * k), F16_OPEN);
			hipLaunchKernelGGL(flat16_fill_kernel, dim3(grid_for(nc)), dim3(256), 0, st, d_T, (long long)nc, F16_OPEN);
			if (ncp > nc)
				hipLaunchKernelGGL(flat16_fill_kernel, dim3(1), dim3(256), 0, st, d_T + nc, (long long)(ncp - nc), 0ull);
			MVS_HIP(hipGetLastError());
			int64_t scap = stream_cap > 0 ? stream_cap
			                              : std::min<int64_t>(F16_MAX_STREAM, std::max<int64_t>({nc * std::min<int64_t>(first, n), nc * k * 4, (int64_t)65536}));
			int64_t a = 0, gen_end = first;
			while (a < n) { // one generation: rows [a, b)
				int64_t b = std::min(n, gen_end);
				unsigned long long cnt = 0;
				for (;;) {
					ws_keys.reserve((size_t)scap * 8);
					ws_recq.reserve((size_t)scap * 4);
					hipLaunchKernelGGL(flat16_fill_kernel, dim3(1), dim3(64), 0, st, d_cnt, 1ll, 0ull);
					F16Scan s;
					memset(&s, 0, sizeof s);
					s.rows = (const uint4 *)words_.p, s.norms = (const float *)norms_.p, s.qf = (const uint4 *)ws_q.p, s.qn = (const float *)ws_qn.p;
					s.T = d_T, s.allow = allow, s.n = n, s.tile0 = a / F16_TILE, s.tile1 = std::min<int64_t>((b + F16_TILE - 1) / F16_TILE, ntiles);
					s.nq = (int)nc, s.S = S, s.l2 = desc ? 0 : 1;
					s.keys = (unsigned long long *)ws_keys.p, s.recq = (uint32_t *)ws_recq.p, s.cnt = d_cnt, s.cap = scap;
					begin_kernel_timing(st);
					grid_last = launch_scan(s, st);
					end_kernel_timing(st);
					++scan_launches;
					const int slot = pinned.acquire(16);
					MVS_HIP(hipMemcpyAsync(pinned.buf[slot], d_cnt, 8, hipMemcpyDeviceToHost, st));
					MVS_HIP(hipStreamSynchronize(st));
					memcpy(&cnt, pinned.buf[slot], 8);
					pinned.release(slot, st);
					if ((int64_t)cnt <= scap)
						break;
					// the stream was too small: nothing of this generation is kept, it runs again with enough room -- or, where even the
					// largest stream would not hold it, as a shorter generation (the next one then scans under a tighter bound)
					++rescans;
					if ((int64_t)cnt <= F16_MAX_STREAM) {
						scap = (int64_t)cnt; // (the scan is deterministic under a fixed bound: the count is exact)
						continue;
					}
					if (b - a <= F16_TILE)
						throw_faiss("mvs::Flat16Index::search", __FILE__, "%llu candidates of one 64-row generation exceed the stream's %lld entries", cnt,
						            (long long)F16_MAX_STREAM);
					b = a + std::max<int64_t>(F16_TILE, (b - a) / 2 / F16_TILE * F16_TILE);
					scap = std::max(scap, std::min<int64_t>(F16_MAX_STREAM, nc * F16_TILE));
				}
				candidates += (int64_t)cnt;
				++generations;
				if (cnt > 0)
					merge_generation((int64_t)cnt, nc, (int)k, K2, d_T, d_qcnt, d_qoff, d_qfill, st);
				a = b;
				gen_end = b * F16_GROWTH;
			}
			hipLaunchKernelGGL(flat16_emit_kernel, dim3(grid_for(nc * k)), dim3(256), 0, st, (const unsigned long long *)ws_best.p, (long long)(nc * k), desc,
			                   map, (long long)label_offset, d_D + (size_t)q0 * k, (long long *)d_I + (size_t)q0 * k);
			MVS_HIP(hipGetLastError());
		}
		set_kinfo(S <= 4 ? "flat16_scan_reg_kernel" : "flat16_scan_lds_kernel", 2.0 * (double)nq * (double)n * 32.0 * S,
		          (double)n * (64.0 * S + 4.0) * (double)((nq + 255) / 256), grid_last, 256, S <= 4 ? 0 : S * 2048, generations);
		stream_wait(stream, st); // (an add that follows on the index's stream waits for the search)
	}

	// ---- reconstruct: the word formula of the file header, decoded by recon_gather_kernel<RECON_F16>
	void recon_source(ReconSource &src, hipStream_t st) override {
		use_device();
		stream_wait(st, stream);
		src.mode = RECON_F16;
		src.rows = words_.p;
		src.pitch = 0;
		src.f16_steps = S;
		src.nrows = ntotal;
		src.push_stage({nullptr, nullptr, (long long)ntotal, (long long)label_offset});
		src.own(stream);
	}
	// ---- images and placement: the host image is a Flat image of the decoded rows, as faiss-gpu's index_gpu_to_cpu gives
	void to_host(HostIndex &out) override {
		out.kind = MVS_KIND_FLAT;
		out.d = d, out.metric = metric, out.metric_arg = metric_arg;
		out.ntotal = ntotal;
		out.is_trained = true;
		out.rows.resize((size_t)ntotal * d);
		if (ntotal > 0)
			reconstruct_n(label_offset, ntotal, out.rows.data());
	}
	IndexBase *clone(int on_device) override { // (a clone without the option: an ordinary Flat index)
		check_device(on_device);
		HostIndex h;
		to_host(h);
		return index_from_host(h, on_device);
	}
	void to_device(int new_device) override {
		if (new_device != device)
			f16_refuse("half-precision Flat on another device (one GPU; clone the Flat source there with use_float16)");
	}

	// ---- refusals
	void range_search(int64_t, const float *, float, const mvs_search_params *, RangeResult &) override {
		f16_refuse("range_search over half-precision Flat");
	}
	void range_search_mapped(int64_t, const float *, float, const mvs_search_params *, const int64_t *, RangeResult &, hipStream_t) override {
		f16_refuse("range_search over half-precision Flat");
	}
	int64_t remove_ids(const mvs_search_params *, const int64_t *, RemoveMarks *) override {
		f16_refuse("remove_ids over half-precision Flat");
	}
	void check_compatible_for_merge(IndexBase &) override {
		f16_refuse("merge_from over half-precision Flat");
	}
	void merge_from(IndexBase &, int64_t) override {
		f16_refuse("merge_from over half-precision Flat");
	}

	bool set_option(const char *key, int64_t v) override {
		if (!strcmp(key, "flat16_first_rows")) {
			if (v < 1)
				throw_faiss("mvs::Flat16Index::set_option", __FILE__, "flat16_first_rows = %lld: at least 1", (long long)v);
			first_rows = v;
			return true;
		}
		if (!strcmp(key, "flat16_stream_cap")) {
			if (v < 0 || v > F16_MAX_STREAM)
				throw_faiss("mvs::Flat16Index::set_option", __FILE__, "flat16_stream_cap = %lld: 0 (automatic) .. %lld", (long long)v,
				            (long long)F16_MAX_STREAM);
			stream_cap = v;
			return true;
		}
		return false;
	}
	bool named_stat(const char *name, int64_t *v) override {
		if (!strcmp(name, "flat16_device_bytes"))
			*v = (int64_t)device_bytes();
		else if (!strcmp(name, "flat16_scan_launches"))
			*v = scan_launches;
		else if (!strcmp(name, "flat16_candidates"))
			*v = candidates;
		else if (!strcmp(name, "flat16_rescans"))
			*v = rescans;
		else
			return false;
		return true;
	}

private:
	DevMem words_, norms_; // [cap / 16][S][64] 16-byte words | [cap] f32
	int64_t cap = 0;       // rows allocated (whole tiles)
	int64_t first_rows = 256, stream_cap = 0;             // options flat16_first_rows / flat16_stream_cap
	int64_t scan_launches = 0, candidates = 0, rescans = 0; // of the last search (the first two) / of the index's life
	DevBuf ws_add, ws_q, ws_qn, ws_best, ws_ctl, ws_keys, ws_recq, ws_seg, ws_temp, ws_allow;
	SelectorHolder selector;

	// -> the grid's workgroups
	int launch_scan(F16Scan &s, hipStream_t st) {
		const long long ntiles = s.tile1 - s.tile0;
		if (ntiles <= 0)
			return 0;
		if (S <= 4) {
			s.nqw = s.nq > 128 ? 4 : (s.nq > 64 ? 2 : 1);
			const int nrl = 4 / s.nqw;
			const long long gx = (s.nq + 64 * s.nqw - 1) / (64 * s.nqw);
			// a few thousand workgroups, query blocks next to each other in dispatch order: the blocks that walk a tile run at the same time
			const long long gy = std::max<long long>(1, std::min<long long>({(ntiles + nrl - 1) / nrl, std::max<long long>(1, 4096 / gx), 65535ll}));
			const dim3 grid((unsigned)gx, (unsigned)gy);
			switch (S) {
			case 1:
				hipLaunchKernelGGL(flat16_scan_reg_kernel<1>, grid, dim3(256), 0, st, s);
				break;
			case 2:
				hipLaunchKernelGGL(flat16_scan_reg_kernel<2>, grid, dim3(256), 0, st, s);
				break;
			case 3:
				hipLaunchKernelGGL(flat16_scan_reg_kernel<3>, grid, dim3(256), 0, st, s);
				break;
			default:
				hipLaunchKernelGGL(flat16_scan_reg_kernel<4>, grid, dim3(256), 0, st, s);
				break;
			}
			MVS_HIP(hipGetLastError());
			return (int)(gx * gy);
		}
		s.nqw = 1;
		const long long gx = (s.nq + 31) / 32;
		const long long gy = std::max<long long>(1, std::min<long long>({(ntiles + 3) / 4, std::max<long long>(1, 4096 / gx), 65535ll}));
		const size_t lds = (size_t)S * 2048;
		ensure_dynamic_lds((const void *)flat16_scan_lds_kernel, lds);
		hipLaunchKernelGGL(flat16_scan_lds_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), lds, st, s);
		MVS_HIP(hipGetLastError());
		return (int)(gx * gy);
	}
	// the records of one generation join their queries' lists: per-query counts, offsets, segments, the select; the bound follows
	void merge_generation(int64_t cnt, int64_t nc, int k, int K2, unsigned long long *d_T, unsigned *d_qcnt, unsigned *d_qoff, unsigned *d_qfill,
	                      hipStream_t st) {
		ws_seg.reserve((size_t)cnt * 8);
		// (d_qcnt | d_qoff | d_qfill are one block of 3 (nc + 1) words: cleared by a kernel, as everything a search clears)
		hipLaunchKernelGGL(flat16_fill_kernel, dim3(grid_for(3 * (nc + 1) / 2 + 1)), dim3(256), 0, st, (unsigned long long *)d_qcnt,
		                   (long long)((3 * (nc + 1) + 1) / 2), 0ull);
		hipLaunchKernelGGL(flat16_hist_kernel, dim3(grid_for(cnt)), dim3(256), 0, st, (const uint32_t *)ws_recq.p, (long long)cnt, d_qcnt);
		size_t temp_bytes = 0;
		MVS_HIP(rocprim::exclusive_scan(nullptr, temp_bytes, d_qcnt, d_qoff, 0u, (size_t)(nc + 1), rocprim::plus<unsigned>(), st));
		ws_temp.reserve(std::max<size_t>(temp_bytes, 16));
		MVS_HIP(rocprim::exclusive_scan(ws_temp.p, temp_bytes, d_qcnt, d_qoff, 0u, (size_t)(nc + 1), rocprim::plus<unsigned>(), st));
		hipLaunchKernelGGL(flat16_scatter_kernel, dim3(grid_for(cnt)), dim3(256), 0, st, (const unsigned long long *)ws_keys.p,
		                   (const uint32_t *)ws_recq.p, (long long)cnt, (const unsigned *)d_qoff, d_qfill, (unsigned long long *)ws_seg.p);
		hipLaunchKernelGGL(flat16_select_kernel, dim3((unsigned)nc), dim3(256), (size_t)2 * K2 * 8, st, (const unsigned long long *)ws_seg.p,
		                   (const unsigned *)d_qoff, (const unsigned *)d_qcnt, k, K2, (unsigned long long *)ws_best.p, d_T);
		MVS_HIP(hipGetLastError());
	}
};

} // namespace

// ---------------------------------------------------------------------------------------------- the clone with use_float16
// `top` is a Flat index or IDMap / IDMap2 over one, under L2 or inner product (the caller has checked).  The clone is built on `device` from
// the source's rows, chunk by chunk: FlatIndex's storage format undone into a scratch of f32 rows (launch_unpack_rows), then the add path
// above -- and, under IDMap, the wrapper's own add_with_ids_device with the source's id map.  Nothing passes through host memory
IndexBase *flat16_clone(IndexBase *top, int device) {
	check_device(device);
	if (top->d > F16_MAX_D) {
		char what[96];
		snprintf(what, sizeof what, "half-precision Flat with d = %d (at most %d dimensions)", top->d, F16_MAX_D);
		f16_refuse(what);
	}
	std::unique_ptr<IndexBase> moved; // the source's plain clone on `device`, where the source lives elsewhere
	if (top->device != device) {
		moved.reset(top->clone(device));
		top = moved.get();
	}
	IDMapIndex *map = top->kind == MVS_KIND_IDMAP ? static_cast<IDMapIndex *>(top) : nullptr;
	FlatIndex *flat = static_cast<FlatIndex *>(map ? map->sub : top);
	flat->use_device();
	flat->flush_adds();
	if (map) {
		map->flush_ids();
		stream_wait(flat->stream, map->stream);
	}
	CtorDevice scope(device);
	Flat16Index *f16 = new Flat16Index(flat->d, flat->metric);
	std::unique_ptr<IndexBase> out(f16);
	f16->metric_arg = flat->metric_arg;
	f16->label_offset = flat->label_offset;
	if (map) {
		IDMapIndex *m = new IDMapIndex(f16);
		out.release();
		out.reset(m);
		m->is_idmap2 = map->is_idmap2;
	}
	const int64_t n = flat->ntotal;
	f16->use_device();
	f16->reserve_rows(n);
	const int64_t chunk = std::max<int64_t>(F16_TILE, ((int64_t)256 << 20) / ((int64_t)flat->d * 4) / F16_TILE * F16_TILE);
	DevBuf rows;
	rows.reserve((size_t)std::min(chunk, std::max<int64_t>(n, 1)) * flat->d * sizeof(float));
	hipStream_t st = flat->stream;
	for (int64_t r0 = 0; r0 < n; r0 += chunk) {
		const int64_t nc = std::min(chunk, n - r0);
		launch_unpack_rows(flat->geom, flat->vecs(), r0, 1, nc, (float *)rows.p, st);
		if (map)
			out->add_with_ids_device(nc, (const float *)rows.p, map->ids.get() + r0, st);
		else
			out->add_device(nc, (const float *)rows.p, st);
	}
	MVS_HIP(hipStreamSynchronize(st)); // (`rows` is freed at scope exit; the source may change again)
	return out.release();
}

void launch_mfma_f16_probe(const unsigned short *d_A, const unsigned short *d_Bt, const float *d_C, float *d_D, int64_t ntiles, hipStream_t st) {
	if (ntiles <= 0)
		return;
	hipLaunchKernelGGL(mfma_f16_probe_kernel, dim3((unsigned)ntiles), dim3(64), 0, st, d_A, d_Bt, d_C, d_D);
	MVS_HIP(hipGetLastError());
}

} // namespace mvs
