// csrc/bf_knn.hip -- faiss::gpu::bfKnn: brute-force k-NN over matrices the CALLER owns, no index (mvs_bf_knn; the contract is the
// "brute-force k-NN on caller-owned matrices" section of include/mi355_faiss.h, the design and the measurements are DESIGN.md 3.20).
//
// fp16 vectors are scanned where they lie.  The arithmetic is half-precision Flat's (csrc/flat_f16.hip): the same operands in the same
// v_mfma_f32_16x16x32_f16 chain, the same test, record stream and select kernels (csrc/flat16_select.h, compiled here as there), so the
// results are the bits of a useFloat16 clone of the same rows.  What is new is how a 16-row operand gets from a dense matrix into the 8
// halves a lane feeds one k-step (lane l: row l & 15, components 32 s + 8 (l >> 4) .. + 7), without a repacked copy:
//   BF_ROW_DIRECT  row-major, d % 8 == 0, base 16-byte aligned: the lane's 8 halves are ONE aligned 16-byte global load at
//                  (row d + 32 s + 8 g) halves; a group of 8 at or beyond d is not loaded, it is zero.
//   BF_ROW_STAGED  row-major, any d and base: per k-step a wave copies, for each of the tile's 64 rows, the aligned hull of the row's
//                  64-byte segment (at most five 16-byte words; a word is loaded iff it holds a byte of the segment, so no load leaves the
//                  matrix's pages) into its own LDS slab at a pitch of 80 bytes.  A lane reads five aligned dwords at its segment offset,
//                  shifts by 16 bits where the offset is odd in halves, and clears the halves at and beyond d.
//   BF_COL_DIRECT  column-major, n % 8 == 0, base aligned: column k of a tile is 128 contiguous bytes = eight 16-byte words; a wave
//                  fetches 8 columns per load instruction (4 per k-step) and writes each word's 8 halves TRANSPOSED into the slab as
//                  [64 rows][32 k] at a pitch of 72 bytes, so the operand is two ds_read_b64 per lane.
//   BF_COL_STAGED  column-major, any n and base: one 2-byte load per lane per column (a column is still one 128-byte request), the same
//                  slab.  Columns at and beyond d and rows at and beyond n are written as zeros.
// The slab is transposed at WRITE time with plain ds_write_b16 into a padded pitch; gfx950's transposing read (ds_read_b64_tr_b16) was not
// used: DESIGN.md 3.20 says why.  A slab belongs to one wave: no workgroup barrier in the tile loop, a wavefront fence orders the slab's
// writes and reads.
//
// Work split, as half-precision Flat's: BF_ROW_DIRECT at d <= 128 keeps a wave's 64 queries in registers (bf_scan_kernel<S, ..>); above
// that, and for the three layouts that go through a slab at every d, a workgroup's 32 queries sit in LDS in fragment order
// (bf_scan_kernel<0, ..>: with a slab's traffic in the loop the register-resident form spilled); waves walk 64-row tiles with a grid
// stride; a result lane holds 4 rows of one query.  Here the k-steps are the outer loop of a tile (an operand is fetched once and meets
// every query group), so all 4 x 4 (4 x 2) accumulators of a tile are live.  k == -1 is the template flag ALL: the 4 scores of a lane are
// stored instead of tested.
//
// bf16 vectors are scanned where they lie too.  An element is still 2 bytes, so the four layouts above move bf16 bits unchanged; the scan
// is a second family of instantiations (bf_scan_kernel<.., BF16 = true>) on v_mfma_f32_16x16x32_bf16, fed by kernels of its own:
// bf_pack_queries_bf16_kernel rounds queries of any type to bf16 in integer arithmetic, bf_qnorm_bf16_kernel and bf_row_norm_bf16_kernel
// decode bits << 16.  The test, the record stream and the select kernels are the fp16 scan's, unchanged.
//
// f32 vectors are not scanned here: they are copied into a transient Flat index on the device (column-major through a transposing kernel)
// and searched by its exact path.
#include "flat16_select.h"

#include <rocprim/device/device_scan.hpp>

#include <cstring>
#include <memory>

#pragma clang fp contract(off)

namespace mvs {

namespace {

enum { BF_ROW_DIRECT = 0, BF_ROW_STAGED = 1, BF_COL_DIRECT = 2, BF_COL_STAGED = 3 };
constexpr int BF_SLAB = 5120;      // bytes of a wave's staging slab: 64 rows x 80 (row-major hull) >= 64 rows x 72 (transposed columns)
constexpr int BF_ROW_PITCH = 80;   // five 16-byte hull words
constexpr int BF_COL_PITCH = 72;   // 32 halves + 8 bytes: rows 18 dwords apart, 8-byte aligned
const char *const FN_BFKNN = "void faiss::gpu::bfKnn(GpuResourcesProvider*, const GpuDistanceParams&)";

constexpr int BF_NORM_KC = 64;     // components of a row per staging round of bf_row_norm_bf16_kernel
constexpr int BF_NORM_PITCH = 66;  // halves: rows 33 dwords apart, so the 64 lanes of a wave read 64 different banks

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct BfScan {
	F16Scan f;               // (rows and allow are null: the operands come from x, every row is allowed)
	const unsigned short *x; // the caller's fp16 or bf16 matrix
	int d;
	float *all;              // ALL: [nq][n] scores of this chunk's queries
};

__device__ __forceinline__ void bf_slab_fence() { // the slab's writes before its reads, its reads before the next writes: one wave, in order
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------------------------- element access, any type and layout
__device__ __forceinline__ float bf16_f32(unsigned bits) { // the decode of a bf16 value: exact
	return __uint_as_float(bits << 16);
}
// element idx of a matrix of type MVS_DIST_*, widened to f32 (exact for the two 16-bit types)
__device__ __forceinline__ float bf_elem_f32(const void *p, int type, long long idx) {
	if (type == MVS_DIST_F16)
		return __half2float(__ushort_as_half(((const unsigned short *)p)[idx]));
	if (type == MVS_DIST_BF16)
		return bf16_f32(((const unsigned short *)p)[idx]);
	return ((const float *)p)[idx];
}
__device__ __forceinline__ unsigned bf_half_bits(const void *p, int type, long long idx) {
	if (type == MVS_DIST_F16)
		return ((const unsigned short *)p)[idx];
	return __half_as_ushort(__float2half_rn(bf_elem_f32(p, type, idx))); // round to nearest even, as flat16_pack_kernel
}
// f32 -> bf16, round to nearest even on the upper 16 bits, in integers: a carry out of the mantissa moves into the exponent (an overflow
// ends at +-inf), subnormals are numbers like any other, and a NaN keeps its upper bits and is quieted: rounding it could reach +-inf
__device__ __forceinline__ unsigned bf_bf16_bits(const void *p, int type, long long idx) {
	if (type == MVS_DIST_BF16)
		return ((const unsigned short *)p)[idx];
	const unsigned b = __float_as_uint(bf_elem_f32(p, type, idx));
	if ((b & 0x7FFFFFFFu) > 0x7F800000u)
		return (b >> 16) | 0x40u;
	return (b + 0x7FFFu + ((b >> 16) & 1u)) >> 16;
}
// queries [q0, q0 + nc) of the caller's matrix -> fragment-major words of 8 fp16 (BF16: bf16) values (the layout of csrc/flat_f16.hip's
// store), padded with zero rows to ncp and with zero components to 32 S.  One thread per 16-byte word
template <bool BF16>
__device__ __forceinline__ void bf_pack_queries(const void *__restrict__ xq, int type, int row_major, long long nq, int d, int S, long long q0,
                                                long long nc, long long ncp, uint4 *__restrict__ words) {
	const long long total = ncp / 16 * S * 64;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const int lane = (int)(i & 63);
		const long long gs = i >> 6, grp = gs / S;
		const int s = (int)(gs % S);
		const long long q = grp * 16 + (lane & 15);
		const int k0 = 32 * s + 8 * (lane >> 4);
		unsigned h[8];
#pragma unroll
		for (int e = 0; e < 8; ++e) {
			const long long idx = row_major ? (q0 + q) * d + k0 + e : (long long)(k0 + e) * nq + q0 + q;
			h[e] = q < nc && k0 + e < d ? (BF16 ? bf_bf16_bits(xq, type, idx) : bf_half_bits(xq, type, idx)) : 0u;
		}
		words[i] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
	}
}
__global__ __launch_bounds__(256) void bf_pack_queries_kernel(const void *__restrict__ xq, int type, int row_major, long long nq, int d, int S,
                                                              long long q0, long long nc, long long ncp, uint4 *__restrict__ words) {
	bf_pack_queries<false>(xq, type, row_major, nq, d, S, q0, nc, ncp, words);
}
__global__ __launch_bounds__(256) void bf_pack_queries_bf16_kernel(const void *__restrict__ xq, int type, int row_major, long long nq, int d, int S,
                                                                   long long q0, long long nc, long long ncp, uint4 *__restrict__ words) {
	bf_pack_queries<true>(xq, type, row_major, nq, d, S, q0, nc, ncp, words);
}
// m_q over the packed bf16 queries: flat16_norm_kernel's chain (k ascending from +0, the padding's zeros leave it as it is) with the
// bf16 decode.  One thread per query
__global__ __launch_bounds__(256) void bf_qnorm_bf16_kernel(const uint4 *__restrict__ words, int S, long long n, float *__restrict__ out) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
		const uint4 *wp = words + (i >> 4) * S * 64 + (i & 15);
		float acc = 0.f;
		for (int s = 0; s < S; ++s)
			for (int g = 0; g < 4; ++g) {
				const uint4 w = wp[s * 64 + g * 16];
				const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
				for (int e = 0; e < 4; ++e) {
					const float lo = bf16_f32(u[e] & 0xFFFFu), hi = __uint_as_float(u[e] & 0xFFFF0000u);
					acc = fmaf(lo, lo, acc);
					acc = fmaf(hi, hi, acc);
				}
			}
		out[i] = acc;
	}
}
// n_i of the caller's bf16 rows, the same chain; rows [n, 64 ntiles) get 0.  A wave per 64-row tile, lane l owns row l of it.  Column-major:
// the lanes' loads of one component are 128 contiguous bytes.  Row-major: BF_NORM_KC components at a time go through the wave's LDS slab
// (lanes along a row: one 128-byte request a row) and each lane then walks its own row there, k ascending
__global__ __launch_bounds__(256) void bf_row_norm_bf16_kernel(const unsigned short *__restrict__ x, int row_major, long long n, long long ntiles, int d,
                                                               float *__restrict__ out) {
	extern __shared__ __attribute__((aligned(16))) unsigned char bf_lds[]; // row-major: 4 slabs of 64 x BF_NORM_PITCH halves; column-major: none
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	unsigned short *slab = reinterpret_cast<unsigned short *>(bf_lds) + w * 64 * BF_NORM_PITCH;
	for (long long tile = (long long)blockIdx.x * 4 + w; tile < ntiles; tile += (long long)gridDim.x * 4) { // (uniform over the wave)
		const long long rowt = tile * 64, row = rowt + lane;
		float acc = 0.f;
		if (!row_major) {
			if (row < n)
#pragma unroll 8
				for (int k = 0; k < d; ++k) {
					const float v = bf16_f32(x[(long long)k * n + row]);
					acc = fmaf(v, v, acc);
				}
		} else {
			const int nr = (int)min(64ll, n - rowt);
			for (int k0 = 0; k0 < d; k0 += BF_NORM_KC) {
				const int kw = min(BF_NORM_KC, d - k0);
				bf_slab_fence();
				if (lane < kw)
#pragma unroll 8
					for (int r = 0; r < nr; ++r)
						slab[r * BF_NORM_PITCH + lane] = x[(rowt + r) * d + k0 + lane];
				bf_slab_fence();
				if (row < n)
					for (int kk = 0; kk < kw; ++kk) {
						const float v = bf16_f32(slab[lane * BF_NORM_PITCH + kk]);
						acc = fmaf(v, v, acc);
					}
			}
		}
		out[row] = acc;
	}
}
// n_i of the caller's fp16 rows: the chain acc = fmaf(v, v, acc) over the decoded halves, k ascending from +0; rows [n, npad) get 0.
// One thread per row (column-major: coalesced; row-major: a thread walks its own row)
__global__ __launch_bounds__(256) void bf_row_norm_kernel(const unsigned short *__restrict__ x, int row_major, long long n, long long npad, int d,
                                                          float *__restrict__ out) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npad; i += (long long)gridDim.x * blockDim.x) {
		float acc = 0.f;
		if (i < n)
			for (int k = 0; k < d; ++k) {
				const float v = __half2float(__ushort_as_half(x[row_major ? i * d + k : (long long)k * n + i]));
				acc = fmaf(v, v, acc);
			}
		out[i] = acc;
	}
}
__global__ __launch_bounds__(256) void bf_fill_f32_kernel(float *__restrict__ p, long long n, float v) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
		p[i] = v;
}
// rows [r0, r0 + nr) of a matrix of any type and layout -> f32 [nr][d] (fp16 and bf16 widen exactly)
__global__ __launch_bounds__(256) void bf_to_f32_rows_kernel(const void *__restrict__ src, int type, int row_major, long long num, int d, long long r0,
                                                             long long nr, float *__restrict__ dst) {
	// consecutive threads take consecutive rows of one component where the source is column-major, consecutive components otherwise
	const long long total = nr * d;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const long long r = row_major ? i / d : i % nr;
		const int k = (int)(row_major ? i % d : i / nr);
		const long long idx = row_major ? (r0 + r) * d + k : (long long)k * num + r0 + r;
		dst[r * d + k] = bf_elem_f32(src, type, idx);
	}
}
// best pairs (or nothing: every slot open) -> distances, unless ignored, and labels of either width
__global__ __launch_bounds__(256) void bf_emit_kernel(const unsigned long long *__restrict__ best, long long total, int descending, float *__restrict__ D,
                                                      long long *__restrict__ I64, int *__restrict__ I32) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const unsigned long long key = best ? best[i] : F16_OPEN;
		const bool open = key == F16_OPEN;
		const long long row = open ? -1 : (long long)(unsigned)key;
		if (D)
			D[i] = open ? (descending ? -FLT_MAX : FLT_MAX) : pq_unkey((unsigned)(key >> 32), descending);
		if (I64)
			I64[i] = row;
		if (I32)
			I32[i] = (int)row;
	}
}
__global__ __launch_bounds__(256) void bf_narrow_labels_kernel(const long long *__restrict__ in, long long total, int *__restrict__ out) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
		out[i] = (int)in[i];
}

// ---------------------------------------------------------------------------------------------- operands
// af[i] = the lane's 8 halves of row 64 tile + 16 i + col, components 32 s + 8 g .. + 7; zero at and beyond d and for rows at and beyond n
template <int LAY>
__device__ __forceinline__ void bf_operands(const BfScan &a, unsigned char *slab, long long tile, int s, int lane, f16x8 (&af)[4]) {
	const int col = lane & 15, g = lane >> 4, d = a.d;
	const long long n = a.f.n, rowt = tile * 64;
	const int k0 = 32 * s + 8 * g;
	if constexpr (LAY == BF_ROW_DIRECT) {
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const long long row = rowt + 16 * i + col;
			u32x4 v = {0u, 0u, 0u, 0u};
			if (row < n && k0 < d) // (d % 8 == 0: the group of 8 is inside the row or beyond it)
				v = *reinterpret_cast<const u32x4 *>(a.x + row * d + k0);
			af[i] = __builtin_bit_cast(f16x8, v);
		}
		return;
	}
	const unsigned long long base = (unsigned long long)a.x;
	bf_slab_fence();
	if constexpr (LAY == BF_ROW_STAGED) {
		const int kw = min(32, d - 32 * s); // halves of a row inside this k-step
#pragma unroll
		for (int t = 0; t < 5; ++t) {
			const int idx = lane + 64 * t, r = idx / 5, j = idx - 5 * r;
			const long long row = rowt + r;
			u32x4 v = {0u, 0u, 0u, 0u};
			if (row < n) {
				const unsigned long long seg = base + ((unsigned long long)row * d + 32 * s) * 2;
				const unsigned long long word = (seg & ~15ull) + 16 * j;
				if (word < seg + 2 * kw) // the word holds a byte of the segment (word + 16 > seg by construction)
					v = *reinterpret_cast<const u32x4 *>(word);
			}
			*reinterpret_cast<u32x4 *>(slab + r * BF_ROW_PITCH + 16 * j) = v;
		}
		bf_slab_fence();
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const int r = 16 * i + col;
			const unsigned long long seg = base + ((unsigned long long)(rowt + r) * d + 32 * s) * 2;
			const int off = r * BF_ROW_PITCH + (int)(seg & 15) + 16 * g;
			const unsigned *p = reinterpret_cast<const unsigned *>(slab + (off & ~3));
			unsigned u[5];
#pragma unroll
			for (int j = 0; j < 5; ++j)
				u[j] = p[j];
			const bool odd = off & 2;
			u32x4 v;
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const unsigned w = odd ? (u[j] >> 16) | (u[j + 1] << 16) : u[j];
				const unsigned keep = (k0 + 2 * j < d ? 0xFFFFu : 0u) | (k0 + 2 * j + 1 < d ? 0xFFFF0000u : 0u);
				v[j] = w & keep;
			}
			af[i] = __builtin_bit_cast(f16x8, v);
		}
		return;
	}
	unsigned short *sh = reinterpret_cast<unsigned short *>(slab);
	if constexpr (LAY == BF_COL_DIRECT) {
#pragma unroll
		for (int t = 0; t < 4; ++t) {
			const int kk = 8 * t + (lane >> 3), r0 = 8 * (lane & 7), k = 32 * s + kk;
			u32x4 v = {0u, 0u, 0u, 0u};
			if (k < d && rowt + r0 < n) // (n % 8 == 0: the word's 8 rows are inside the column or beyond it)
				v = *reinterpret_cast<const u32x4 *>(a.x + (long long)k * n + rowt + r0);
#pragma unroll
			for (int e = 0; e < 8; ++e)
				sh[(r0 + e) * (BF_COL_PITCH / 2) + kk] = (unsigned short)(e & 1 ? v[e >> 1] >> 16 : v[e >> 1] & 0xFFFFu);
		}
	} else {
		const long long row = rowt + lane;
#pragma unroll
		for (int kk = 0; kk < 32; ++kk) {
			const int k = 32 * s + kk;
			unsigned short v = 0;
			if (k < d && row < n)
				v = a.x[(long long)k * n + row];
			sh[lane * (BF_COL_PITCH / 2) + kk] = v;
		}
	}
	bf_slab_fence();
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const uint2 *p = reinterpret_cast<const uint2 *>(slab + (16 * i + col) * BF_COL_PITCH + 16 * g);
		const uint2 lo = p[0], hi = p[1];
		af[i] = __builtin_bit_cast(f16x8, (u32x4) {lo.x, lo.y, hi.x, hi.y});
	}
}

// ALL: the 4 scores of a lane go to out[q][row4 ..]; no rule, no bound
__device__ __forceinline__ void bf_store4(const BfScan &a, const f32x4 &acc, float mq, const float4 &nr, long long row4, int q) {
	if (q >= a.f.nq)
		return;
	const float nrm[4] = {nr.x, nr.y, nr.z, nr.w};
#pragma unroll
	for (int r = 0; r < 4; ++r) {
		float s = acc[r];
		if (a.f.l2) {
			s = fmaf(-2.f, s, mq + nrm[r]);
			s = s < 0.f ? 0.f : s;
		}
		if (row4 + r < a.f.n)
			a.all[(size_t)q * a.f.n + row4 + r] = s;
	}
}

// ---------------------------------------------------------------------------------------------- scan
// SREG > 0: d <= 128, SREG k-steps, a wave's 64 queries in registers (NJ = 4 groups of 16).  SREG == 0: the workgroup's 32 queries in
// LDS as [S][2][64] words behind the slabs (NJ = 2), the 4 waves on different tiles.  Dynamic LDS: 4 slabs where LAY stages, then the queries
// BF16 picks the instruction: fragments travel as 16 bytes of bits (f16x8 is their carrier, not their arithmetic).  The kernel itself
// takes the flag, not a shared body under two kernels: that form rescheduled the fp16 instantiations, this one leaves their instruction
// streams as they were without it
template <bool BF16>
__device__ __forceinline__ f32x4 bf_mfma(f16x8 rows, f16x8 queries, f32x4 acc) {
	if constexpr (BF16)
		return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, rows), __builtin_bit_cast(bf16x8, queries), acc, 0, 0, 0);
	else
		return __builtin_amdgcn_mfma_f32_16x16x32_f16(rows, queries, acc, 0, 0, 0);
}
template <int SREG, int LAY, bool ALL, bool BF16>
__global__ __launch_bounds__(256, 2) void bf_scan_kernel(const BfScan a) {
	extern __shared__ __attribute__((aligned(16))) unsigned char bf_lds[];
	constexpr int NJ = SREG ? 4 : 2, SQ = SREG ? SREG : 1;
	constexpr bool STAGED = LAY != BF_ROW_DIRECT;
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
	unsigned char *slab = bf_lds + (STAGED ? w * BF_SLAB : 0);
	const uint4 *qlds = reinterpret_cast<const uint4 *>(bf_lds + (STAGED ? 4 * BF_SLAB : 0));
	const int S = SREG ? SREG : a.f.S;
	int q0;
	long long tile, step;
	f16x8 qf[NJ][SQ];
	if constexpr (SREG > 0) {
		const int qwave = w % a.f.nqw, rl = w / a.f.nqw, nrl = 4 / a.f.nqw;
		q0 = (blockIdx.x * a.f.nqw + qwave) * 64;
		if (q0 >= a.f.nq)
			return; // (uniform over the wave; this instantiation has no workgroup barrier)
		tile = a.f.tile0 + (long long)blockIdx.y * nrl + rl, step = (long long)gridDim.y * nrl;
#pragma unroll
		for (int j = 0; j < 4; ++j)
#pragma unroll
			for (int s = 0; s < SREG; ++s)
				qf[j][s] = *reinterpret_cast<const f16x8 *>(a.f.qf + ((size_t)((q0 >> 4) + j) * SREG + s) * 64 + lane);
	} else {
		q0 = blockIdx.x * 32;
		uint4 *qw = reinterpret_cast<uint4 *>(bf_lds + (STAGED ? 4 * BF_SLAB : 0));
		for (int i = threadIdx.x; i < S * 128; i += 256) {
			const int s = i >> 7, j = (i >> 6) & 1, ln = i & 63;
			qw[i] = a.f.qf[((size_t)((q0 >> 4) + j) * S + s) * 64 + ln];
		}
		__syncthreads();
		tile = a.f.tile0 + (long long)blockIdx.y * 4 + w, step = (long long)gridDim.y * 4;
	}
	F16Bound bd[NJ];
#pragma unroll
	for (int j = 0; j < NJ; ++j) {
		if constexpr (ALL)
			bd[j].t = 0, bd[j].tb = 0.f, bd[j].mq = a.f.qn[q0 + 16 * j + col];
		else
			bd[j] = f16_bound(a.f, q0 + 16 * j + col);
	}
	for (; tile < a.f.tile1; tile += step) {
		f32x4 acc[4][NJ];
#pragma unroll
		for (int i = 0; i < 4; ++i)
#pragma unroll
			for (int j = 0; j < NJ; ++j)
				acc[i][j] = f32x4 {0.f, 0.f, 0.f, 0.f};
		if constexpr (SREG > 0) {
#pragma unroll
			for (int s = 0; s < SREG; ++s) {
				f16x8 af[4];
				bf_operands<LAY>(a, slab, tile, s, lane, af);
#pragma unroll
				for (int i = 0; i < 4; ++i)
#pragma unroll
					for (int j = 0; j < 4; ++j)
						acc[i][j] = bf_mfma<BF16>(af[i], qf[j][s], acc[i][j]);
			}
		} else {
			for (int s = 0; s < S; ++s) {
				f16x8 af[4];
				bf_operands<LAY>(a, slab, tile, s, lane, af);
				const f16x8 b0 = *reinterpret_cast<const f16x8 *>(qlds + (s * 2 + 0) * 64 + lane);
				const f16x8 b1 = *reinterpret_cast<const f16x8 *>(qlds + (s * 2 + 1) * 64 + lane);
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					acc[i][0] = bf_mfma<BF16>(af[i], b0, acc[i][0]);
					acc[i][1] = bf_mfma<BF16>(af[i], b1, acc[i][1]);
				}
			}
		}
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const long long row4 = tile * 64 + 16 * i + 4 * g;
			const float4 nr = *reinterpret_cast<const float4 *>(a.f.norms + row4); // (the norms are padded to whole tiles)
#pragma unroll
			for (int j = 0; j < NJ; ++j) {
				if constexpr (ALL)
					bf_store4(a, acc[i][j], bd[j].mq, nr, row4, q0 + 16 * j + col);
				else
					f16_test4(a.f, acc[i][j], bd[j], nr, row4, q0 + 16 * j + col, ~0ull, 16 * i + 4 * g, lane);
			}
		}
	}
}

typedef void (*bf_scan_fn)(const BfScan);
template <int SREG, int LAY, bool ALL>
bf_scan_fn bf_scan_of(bool bf16) {
	return bf16 ? bf_scan_kernel<SREG, LAY, ALL, true> : bf_scan_kernel<SREG, LAY, ALL, false>;
}
template <int LAY, bool ALL>
bf_scan_fn bf_scan_for_steps(bool bf16, int S) {
	switch (S) {
	case 1:
		return bf_scan_of<1, LAY, ALL>(bf16);
	case 2:
		return bf_scan_of<2, LAY, ALL>(bf16);
	case 3:
		return bf_scan_of<3, LAY, ALL>(bf16);
	case 4:
		return bf_scan_of<4, LAY, ALL>(bf16);
	default:
		return bf_scan_of<0, LAY, ALL>(bf16);
	}
}
// the register-resident instantiations exist for BF_ROW_DIRECT alone: with a slab's traffic in the loop they spill
template <bool ALL>
bf_scan_fn bf_scan_for(bool bf16, int lay, int S) {
	switch (lay) {
	case BF_ROW_DIRECT:
		return bf_scan_for_steps<BF_ROW_DIRECT, ALL>(bf16, S);
	case BF_ROW_STAGED:
		return bf_scan_of<0, BF_ROW_STAGED, ALL>(bf16);
	case BF_COL_DIRECT:
		return bf_scan_of<0, BF_COL_DIRECT, ALL>(bf16);
	default:
		return bf_scan_of<0, BF_COL_STAGED, ALL>(bf16);
	}
}

// the grid of csrc/flat_f16.hip's launch_scan: a few thousand workgroups, query blocks next to each other in dispatch order
void bf_launch_scan(BfScan &s, bool bf16, int lay, bool all, hipStream_t st) {
	const long long ntiles = s.f.tile1 - s.f.tile0;
	if (ntiles <= 0)
		return;
	const int S = s.f.S;
	size_t lds = lay == BF_ROW_DIRECT ? 0 : 4 * BF_SLAB;
	long long gx, gy;
	if (S <= 4 && lay == BF_ROW_DIRECT) {
		s.f.nqw = s.f.nq > 128 ? 4 : (s.f.nq > 64 ? 2 : 1);
		const int nrl = 4 / s.f.nqw;
		gx = (s.f.nq + 64 * s.f.nqw - 1) / (64 * s.f.nqw);
		gy = std::max<long long>(1, std::min<long long>({(ntiles + nrl - 1) / nrl, std::max<long long>(1, 4096 / gx), 65535ll}));
	} else {
		s.f.nqw = 1;
		gx = (s.f.nq + 31) / 32;
		gy = std::max<long long>(1, std::min<long long>({(ntiles + 3) / 4, std::max<long long>(1, 4096 / gx), 65535ll}));
		lds += (size_t)S * 2048;
	}
	const bf_scan_fn fn = all ? bf_scan_for<true>(bf16, lay, S) : bf_scan_for<false>(bf16, lay, S);
	ensure_dynamic_lds((const void *)fn, lds);
	hipLaunchKernelGGL(fn, dim3((unsigned)gx, (unsigned)gy), dim3(256), lds, st, s);
	MVS_HIP(hipGetLastError());
}

[[noreturn]] void bf_refuse(const char *what) {
	throw_faiss(FN_BFKNN, "faiss/gpu/GpuDistance.cpp", "This index type is not implemented on the MI355X path yet: bfKnn %s", what);
}

struct DeviceScope { // the call runs on the params' device and leaves the thread's current device as it found it
	int prev = 0;
	explicit DeviceScope(int dev) {
		MVS_HIP(hipGetDevice(&prev));
		MVS_HIP(hipSetDevice(dev));
	}
	~DeviceScope() {
		(void)hipSetDevice(prev);
	}
};

// ---------------------------------------------------------------------------------------------- fp16 and bf16 vectors: the scan above
// One host path for both 16-bit types: workspaces, generations and selection do not depend on the element type; the norm, pack and scan
// kernels do, and are chosen by it
void bf_knn_scan(const mvs_distance_params &p, hipStream_t st) {
	const int d = p.dims, S = (d + 31) / 32, desc = p.metric == METRIC_L2 ? 0 : 1;
	const bool all = p.k == -1, bf16 = p.vector_type == MVS_DIST_BF16;
	const int64_t n = p.num_vectors, nq = p.num_queries, k = p.k;
	const int64_t ntiles = (n + F16_TILE - 1) / F16_TILE, npad = ntiles * F16_TILE;
	const unsigned short *x = (const unsigned short *)p.vectors;
	const bool aligned = ((uintptr_t)x & 15) == 0;
	const int lay = p.vectors_row_major ? (aligned && d % 8 == 0 ? BF_ROW_DIRECT : BF_ROW_STAGED) : (aligned && n % 8 == 0 ? BF_COL_DIRECT : BF_COL_STAGED);
	int *I32 = p.out_indices_type == MVS_IDX_I32 ? (int *)p.out_indices : nullptr;
	long long *I64 = p.out_indices_type == MVS_IDX_I32 ? nullptr : (long long *)p.out_indices;
	float *D = p.ignore_out_distances ? nullptr : p.out_distances;

	DevBuf ws_norms, ws_q, ws_qn, ws_best, ws_ctl, ws_keys, ws_recq, ws_seg, ws_temp;
	PinnedMem pin;
	pin.reserve(16);
	// n_i: the caller's, verbatim, or the chain; zero for the last tile's padding
	ws_norms.reserve((size_t)npad * sizeof(float));
	if (p.vector_norms) {
		MVS_HIP(hipMemcpyAsync(ws_norms.p, p.vector_norms, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
		if (npad > n)
			hipLaunchKernelGGL(bf_fill_f32_kernel, dim3(1), dim3(64), 0, st, (float *)ws_norms.p + n, (long long)(npad - n), 0.f);
	} else if (bf16) {
		hipLaunchKernelGGL(bf_row_norm_bf16_kernel, dim3(grid_for(ntiles, 4)), dim3(256), p.vectors_row_major ? 4 * 64 * BF_NORM_PITCH * 2 : 0, st, x,
		                   (int)p.vectors_row_major, (long long)n, (long long)ntiles, d, (float *)ws_norms.p);
	} else {
		hipLaunchKernelGGL(bf_row_norm_kernel, dim3(grid_for(npad)), dim3(256), 0, st, x, (int)p.vectors_row_major, (long long)n, (long long)npad, d,
		                   (float *)ws_norms.p);
	}
	MVS_HIP(hipGetLastError());
	int K2 = 256;
	while (K2 < k)
		K2 <<= 1;
	const int64_t first = (std::max<int64_t>(256, k) + F16_TILE - 1) / F16_TILE * F16_TILE; // rows examined before the first bound exists
	for (int64_t q0 = 0; q0 < nq; q0 += F16_QCHUNK) {
		const int64_t nc = std::min(F16_QCHUNK, nq - q0), ncp = (nc + 63) / 64 * 64;
		ws_q.reserve((size_t)ncp * S * 64);
		ws_qn.reserve((size_t)ncp * sizeof(float));
		// the queries as half-precision Flat packs them: rounded to the vectors' type, fragment-major, m_q by the same chain
		const auto pack = bf16 ? bf_pack_queries_bf16_kernel : bf_pack_queries_kernel;
		hipLaunchKernelGGL(pack, dim3(grid_for(ncp / 16 * S * 64)), dim3(256), 0, st, p.queries, (int)p.query_type, (int)p.queries_row_major, (long long)nq,
		                   d, S, (long long)q0, (long long)nc, (long long)ncp, (uint4 *)ws_q.p);
		if (bf16)
			hipLaunchKernelGGL(bf_qnorm_bf16_kernel, dim3(grid_for(ncp)), dim3(256), 0, st, (const uint4 *)ws_q.p, S, (long long)ncp, (float *)ws_qn.p);
		else
			hipLaunchKernelGGL(flat16_norm_kernel, dim3(grid_for(ncp)), dim3(256), 0, st, (const uint4 *)ws_q.p, S, 0ll, (long long)ncp, (float *)ws_qn.p);
		MVS_HIP(hipGetLastError());
		BfScan s;
		memset(&s, 0, sizeof s);
		s.x = x, s.d = d;
		s.f.norms = (const float *)ws_norms.p, s.f.qf = (const uint4 *)ws_q.p, s.f.qn = (const float *)ws_qn.p;
		s.f.n = n, s.f.nq = (int)nc, s.f.S = S, s.f.l2 = desc ? 0 : 1;
		if (all) {
			s.all = p.out_distances + (size_t)q0 * n;
			s.f.tile0 = 0, s.f.tile1 = ntiles;
			bf_launch_scan(s, bf16, lay, true, st);
			continue;
		}
		ws_best.reserve((size_t)nc * k * 8);
		ws_ctl.reserve(64 + (size_t)ncp * 8 + 3 * (size_t)(nc + 1) * 4 + 64);
		unsigned long long *d_cnt = (unsigned long long *)ws_ctl.p;
		unsigned long long *d_T = (unsigned long long *)((char *)ws_ctl.p + 64);
		unsigned *d_qcnt = (unsigned *)(d_T + ncp), *d_qoff = d_qcnt + (nc + 1), *d_qfill = d_qoff + (nc + 1);
		hipLaunchKernelGGL(flat16_fill_kernel, dim3(grid_for(nc * k)), dim3(256), 0, st, (unsigned long long *)ws_best.p, (long long)(nc * k), F16_OPEN);
		hipLaunchKernelGGL(flat16_fill_kernel, dim3(grid_for(nc)), dim3(256), 0, st, d_T, (long long)nc, F16_OPEN);
		if (ncp > nc)
			hipLaunchKernelGGL(flat16_fill_kernel, dim3(1), dim3(256), 0, st, d_T + nc, (long long)(ncp - nc), 0ull);
		MVS_HIP(hipGetLastError());
		int64_t scap = std::min<int64_t>(F16_MAX_STREAM, std::max<int64_t>({nc * std::min<int64_t>(first, n), nc * k * 4, (int64_t)65536}));
		int64_t a = 0, gen_end = first;
		while (a < n) { // one generation: rows [a, b), as Flat16Index::search_mapped
			int64_t b = std::min(n, gen_end);
			unsigned long long cnt = 0;
			for (;;) {
				ws_keys.reserve((size_t)scap * 8);
				ws_recq.reserve((size_t)scap * 4);
				hipLaunchKernelGGL(flat16_fill_kernel, dim3(1), dim3(64), 0, st, d_cnt, 1ll, 0ull);
				s.f.T = d_T, s.f.tile0 = a / F16_TILE, s.f.tile1 = std::min<int64_t>((b + F16_TILE - 1) / F16_TILE, ntiles);
				s.f.keys = (unsigned long long *)ws_keys.p, s.f.recq = (uint32_t *)ws_recq.p, s.f.cnt = d_cnt, s.f.cap = scap;
				bf_launch_scan(s, bf16, lay, false, st);
				MVS_HIP(hipMemcpyAsync(pin.p, d_cnt, 8, hipMemcpyDeviceToHost, st));
				MVS_HIP(hipStreamSynchronize(st));
				memcpy(&cnt, pin.p, 8);
				if ((int64_t)cnt <= scap)
					break;
				// the stream was too small: the generation runs again with enough room, or shorter where no stream would hold it
				if ((int64_t)cnt <= F16_MAX_STREAM) {
					scap = (int64_t)cnt;
					continue;
				}
				if (b - a <= F16_TILE)
					throw_faiss(FN_BFKNN, __FILE__, "%llu candidates of one 64-row generation exceed the stream's %lld entries", cnt, (long long)F16_MAX_STREAM);
				b = a + std::max<int64_t>(F16_TILE, (b - a) / 2 / F16_TILE * F16_TILE);
				scap = std::max(scap, std::min<int64_t>(F16_MAX_STREAM, nc * F16_TILE));
			}
			if (cnt > 0) { // the records join their queries' lists; the bounds follow
				ws_seg.reserve((size_t)cnt * 8);
				hipLaunchKernelGGL(flat16_fill_kernel, dim3(grid_for(3 * (nc + 1) / 2 + 1)), dim3(256), 0, st, (unsigned long long *)d_qcnt,
				                   (long long)((3 * (nc + 1) + 1) / 2), 0ull);
				hipLaunchKernelGGL(flat16_hist_kernel, dim3(grid_for((long long)cnt)), dim3(256), 0, st, (const uint32_t *)ws_recq.p, (long long)cnt, d_qcnt);
				size_t temp_bytes = 0;
				MVS_HIP(rocprim::exclusive_scan(nullptr, temp_bytes, d_qcnt, d_qoff, 0u, (size_t)(nc + 1), rocprim::plus<unsigned>(), st));
				ws_temp.reserve(std::max<size_t>(temp_bytes, 16));
				MVS_HIP(rocprim::exclusive_scan(ws_temp.p, temp_bytes, d_qcnt, d_qoff, 0u, (size_t)(nc + 1), rocprim::plus<unsigned>(), st));
				hipLaunchKernelGGL(flat16_scatter_kernel, dim3(grid_for((long long)cnt)), dim3(256), 0, st, (const unsigned long long *)ws_keys.p,
				                   (const uint32_t *)ws_recq.p, (long long)cnt, (const unsigned *)d_qoff, d_qfill, (unsigned long long *)ws_seg.p);
				hipLaunchKernelGGL(flat16_select_kernel, dim3((unsigned)nc), dim3(256), (size_t)2 * K2 * 8, st, (const unsigned long long *)ws_seg.p,
				                   (const unsigned *)d_qoff, (const unsigned *)d_qcnt, (int)k, K2, (unsigned long long *)ws_best.p, d_T);
				MVS_HIP(hipGetLastError());
			}
			a = b;
			gen_end = b * F16_GROWTH;
		}
		hipLaunchKernelGGL(bf_emit_kernel, dim3(grid_for(nc * k)), dim3(256), 0, st, (const unsigned long long *)ws_best.p, (long long)(nc * k), desc,
		                   D ? D + (size_t)q0 * k : nullptr, I64 ? I64 + (size_t)q0 * k : nullptr, I32 ? I32 + (size_t)q0 * k : nullptr);
		MVS_HIP(hipGetLastError());
	}
	MVS_HIP(hipStreamSynchronize(st)); // (the workspaces go at scope exit)
}

// ---------------------------------------------------------------------------------------------- f32 vectors: a transient Flat index
void bf_knn_f32(const mvs_distance_params &p, hipStream_t st) {
	if (p.k == -1)
		bf_refuse("with k = -1 over f32 vectors (all pairwise distances are served for fp16 and bf16 vectors)");
	const int d = p.dims;
	const int64_t n = p.num_vectors, nq = p.num_queries, k = p.k;
	CtorDevice scope(p.device);
	std::unique_ptr<IndexBase> ix(index_factory(d, "Flat", p.metric));
	DevBuf rows, xq, tmpD, tmpI;
	if (p.vectors_row_major) {
		ix->add_device(n, (const float *)p.vectors, st);
	} else { // transposed chunk by chunk into the index
		const int64_t chunk = std::max<int64_t>(F16_TILE, ((int64_t)256 << 20) / ((int64_t)d * 4));
		rows.reserve((size_t)std::min(chunk, n) * d * sizeof(float));
		for (int64_t r0 = 0; r0 < n; r0 += chunk) {
			const int64_t nr = std::min(chunk, n - r0);
			hipLaunchKernelGGL(bf_to_f32_rows_kernel, dim3(grid_for(nr * d)), dim3(256), 0, st, p.vectors, MVS_DIST_F32, 0, (long long)n, d, (long long)r0,
			                   (long long)nr, (float *)rows.p);
			MVS_HIP(hipGetLastError());
			ix->add_device(nr, (const float *)rows.p, st);
		}
	}
	const float *q = (const float *)p.queries;
	if (p.query_type != MVS_DIST_F32 || !p.queries_row_major) {
		xq.reserve((size_t)nq * d * sizeof(float));
		hipLaunchKernelGGL(bf_to_f32_rows_kernel, dim3(grid_for(nq * d)), dim3(256), 0, st, p.queries, (int)p.query_type, (int)p.queries_row_major,
		                   (long long)nq, d, 0ll, (long long)nq, (float *)xq.p);
		MVS_HIP(hipGetLastError());
		q = (const float *)xq.p;
	}
	float *D = p.out_distances;
	int64_t *I = (int64_t *)p.out_indices;
	if (p.ignore_out_distances) {
		tmpD.reserve((size_t)nq * k * sizeof(float));
		D = (float *)tmpD.p;
	}
	if (p.out_indices_type == MVS_IDX_I32) {
		tmpI.reserve((size_t)nq * k * sizeof(int64_t));
		I = (int64_t *)tmpI.p;
	}
	ix->search_device(nq, q, k, D, I, nullptr, st);
	if (p.out_indices_type == MVS_IDX_I32) {
		hipLaunchKernelGGL(bf_narrow_labels_kernel, dim3(grid_for(nq * k)), dim3(256), 0, st, (const long long *)I, (long long)(nq * k), (int *)p.out_indices);
		MVS_HIP(hipGetLastError());
	}
	MVS_HIP(hipStreamSynchronize(st));
}

void bf_knn(const mvs_distance_params &params) {
	mvs_distance_params p = params;
	if (p.device < 0) // faiss::gpu::GpuDistanceParams::device == -1: the calling thread's current device
		MVS_HIP(hipGetDevice(&p.device));
	if (p.metric != METRIC_L2 && p.metric != METRIC_IP) {
		char what[96];
		snprintf(what, sizeof what, "with metric %d (L2 and inner product only)", p.metric);
		bf_refuse(what);
	}
	if (p.dims < 1)
		throw_faiss(FN_BFKNN, "faiss/gpu/GpuDistance.cpp", "Error: 'args.dims > 0' failed");
	if (p.dims > F16_MAX_D) {
		char what[96];
		snprintf(what, sizeof what, "with d = %d (at most %d dimensions)", p.dims, F16_MAX_D);
		bf_refuse(what);
	}
	if (p.k == 0 || p.k < -1)
		throw_faiss(FN_BFKNN, "faiss/gpu/GpuDistance.cpp", "Error: 'k > 0' failed");
	if (p.k > F16_MAX_K) {
		char what[96];
		snprintf(what, sizeof what, "with k = %d (at most %d)", p.k, F16_MAX_K);
		bf_refuse(what);
	}
	if (p.vector_type < MVS_DIST_F32 || p.vector_type > MVS_DIST_BF16 || p.query_type < MVS_DIST_F32 || p.query_type > MVS_DIST_BF16)
		bf_refuse("with a data type beyond f32, f16 and bf16");
	if (p.out_indices_type != MVS_IDX_I64 && p.out_indices_type != MVS_IDX_I32)
		throw_faiss(FN_BFKNN, "faiss/gpu/GpuDistance.cpp", "Error: unknown outIndicesType %d", p.out_indices_type);
	if (p.num_vectors < 0 || p.num_queries < 0 || p.num_vectors >= ((int64_t)1 << 31))
		throw_faiss(FN_BFKNN, "faiss/gpu/GpuDistance.cpp", "Error: numVectors = %lld, numQueries = %lld: at most 2^31 - 1 vectors", (long long)p.num_vectors,
		            (long long)p.num_queries);
	if (p.num_queries == 0)
		return;
	const bool all = p.k == -1;
	if (!p.queries || (p.num_vectors > 0 && !p.vectors) || (all ? !p.out_distances : !p.out_indices) || (!all && !p.ignore_out_distances && !p.out_distances))
		throw_faiss(FN_BFKNN, "faiss/gpu/GpuDistance.cpp", "Error: a null vectors, queries or output pointer");
	check_device(p.device);
	DeviceScope on(p.device);
	hipStream_t st = (hipStream_t)p.stream;
	if (p.num_vectors == 0) { // nothing to find: every slot is the padding
		if (!all) {
			const long long total = (long long)p.num_queries * p.k;
			const bool i32 = p.out_indices_type == MVS_IDX_I32;
			hipLaunchKernelGGL(bf_emit_kernel, dim3(grid_for(total)), dim3(256), 0, st, (const unsigned long long *)nullptr, total,
			                   p.metric == METRIC_L2 ? 0 : 1, p.ignore_out_distances ? nullptr : p.out_distances, i32 ? nullptr : (long long *)p.out_indices,
			                   i32 ? (int *)p.out_indices : nullptr);
			MVS_HIP(hipGetLastError());
			MVS_HIP(hipStreamSynchronize(st));
		}
		return;
	}
	if (p.vector_type != MVS_DIST_F32)
		bf_knn_scan(p, st);
	else
		bf_knn_f32(p, st);
}

} // namespace

} // namespace mvs

extern "C" int mvs_bf_knn(const mvs_distance_params *p) {
	try {
		if (!p)
			mvs::throw_faiss(mvs::FN_BFKNN, "faiss/gpu/GpuDistance.cpp", "Error: null parameters");
		mvs::bf_knn(*p);
		return 0;
	} catch (const std::exception &e) {
		mvs::set_last_error(e.what());
	} catch (...) {
		mvs::set_last_error("unknown error");
	}
	return 1;
}
