// csrc/flat_collect_big.hip -- the bf16 coarse filter for 512 < d <= 1024 with ALL of k resident in ONE wave: one wavefront per
// SIMD, 512 registers each.
//
// Same argument, bound, candidate stream and re-scoring as flat_collect.hip / flat_collect_wide.hip; only the geometry of the scan
// differs.  The k-split kernel this one replaced (removed; git log has it) split k over a wave pair because 32 queries x 24 k-blocks
// = 192 VGPRs of query fragments do not fit next to the rest in 256 registers at two waves per SIMD; every A fragment read from LDS
// then fed only 2-3 MFMAs, the pair handed partial sums over through LDS behind a workgroup barrier per 16-row tile, and the
// matrix pipe was 36 % busy (the kernel was LDS-read-bound).  A gfx950 wave that runs alone on its SIMD owns 512 registers (256 VGPRs + 256
// AGPRs, one unified file; the MFMA reads its A / B operands from either half), so here
//   wave        NCB column blocks of 16 queries x KBT k-blocks of query fragments RESIDENT: 4 x 24 x 4 = 384 registers at the
//               768-dim store (64 queries per wave), 3 x 32 x 4 = 384 at the 1024-dim store (48 queries); no k split, no
//               hand-over, each ds_read_b128 of an A fragment feeds NCB MFMAs (64 matrix-pipe cycles at NCB = 4).
//               hipcc's MFMA builtin only takes its A / B operands from VGPRs and treats AGPRs as spill space (the first
//               version of this kernel spent 4 v_accvgpr_read per MFMA on half of its fragments), so the 60 fragments placed
//               in AGPRs are consumed by hand-written v_mfma instructions with an AGPR srcB ("a" constraint); the other 36
//               stay with the builtin.  The hand-written ones are invisible to the compiler's hazard recognizer: every
//               accumulator is written once per NCB MFMAs (>= 48 cycles apart) and read by the vector ALU only behind a
//               scheduling barrier one tile later (or behind explicit s_nops after the last tile).
//   workgroup   4 waves = one per SIMD, one workgroup per CU: 256 (192) queries share every tile the CU stages
//   tiles       16 rows x (64 KBT) bytes, a ring of FOUR stages filled by LDS-DMA three tiles ahead.  A lone wave has nobody
//               else to fill its matrix pipe, so nothing may sit between two tiles' MFMAs: the tile's ONE barrier stands in the
//               MIDDLE of its MFMA loop (in front of k-block 8; its s_waitcnt lets the newest block's loads stay in flight),
//               the LDS-DMA instructions of block u + 3 (~100 issue cycles each) are spread one per two k-blocks behind it,
//               and the first fragments (and beta) of tile u + 1 are read from LDS under the last MFMAs of tile u
//   epilogue    running maxima + bound test of tile u - 1 run on the vector ALU behind the first MFMAs of tile u (two
//               accumulator sets, the tile loop unrolled by two)
#include "flat_collect.h"

#include <algorithm>
#include <cstring>
#include <type_traits>

namespace mvs {

typedef float f32x4b __attribute__((ext_vector_type(4)));
__host__ __device__ constexpr int big_stages(int stage_bytes) { // LDS ring of the staged blocks
	(void)stage_bytes; // (five stages at 24 KB blocks -- a block requested FOUR tiles ahead -- measured no different from four: 145.7 vs 145.1 ms at C4)
	return 4;
}


// The next tile's first fragments and beta are read under the last MFMAs of this one; the LDS-DMA instructions of block u + 3
// are spread one per two k-blocks.  (Issuing either behind the barrier instead measured slower; git log has those variants.)
// KSPL (the 1536-dim store: 2): a row is KSPL PARTS of KBT k-blocks; a staged block holds ONE part of 16 rows (the ring, the barrier
// and the LDS-DMA pattern are those of a KBT-wide store with KSPL times the rows), the accumulators run through the parts of a row
// block (the chain starts at beta in part 0) and are tested after the last; all KSPL * KBT k-blocks of query fragments are resident.
// NC: row classes per query (16; 32 for 16 < kk <= 32 -- csrc/flat_collect.hip)
template <int KBT, int NCB, bool IS_L2, bool COLLECT, int KSPL = 1, int NC = 16>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void flat_bf16_big_kernel(const CollectArgs a) {
	constexpr int KT = KBT * KSPL; // k-blocks of a whole row
	constexpr int PITCH = 64 * KBT, GPITCH = PITCH * KSPL, C = 4 * KBT, RT = 16; // bytes of a staged row (one part) / of a stored row
	constexpr int STAGE_BYTES = RT * PITCH; // 24 KB (768 dims) / 32 KB (1024)
	constexpr int NST = big_stages(STAGE_BYTES), KB_BAR = 8; // (the ring's length is a parameter since round 5: see big_stages)
	constexpr int DMA_PER_WAVE = STAGE_BYTES / 4096;
	constexpr int QW = 16 * NCB, QB = 4 * QW;
	constexpr int RA = 4, RING = 8; // A fragments read RA k-blocks ahead into a ring of RING register quads
	constexpr int FLUSH_EVERY = 8;
	static_assert(STAGE_BYTES % 4096 == 0 && KBT % RING == 0 && NCB >= 2 && NCB <= 4 && RA < RING && (KSPL == 1 || KSPL == 2), "geometry");
	static_assert(KB_BAR + 2 * DMA_PER_WAVE < KBT + 1 && KB_BAR < KBT - RA, "the block's LDS-DMA instructions fit behind the barrier");

	extern __shared__ __attribute__((aligned(16))) float smem[];
	char *tbuf = (char *)smem;                                          // [NST][STAGE_BYTES]
	float *nbuf = (float *)(tbuf + NST * STAGE_BYTES);                  // [NST][64] beta of the staged rows (16 used)
	unsigned long long *qbuf = (unsigned long long *)(nbuf + NST * 64); // [CL_QCAP] candidate queue
	float *cqtab = (float *)(qbuf + CL_QCAP);                           // [4 waves][16 c][4]: pass bound of column block i, query c
	unsigned *qctl = (unsigned *)(cqtab + 4 * 16 * 4);                  // [0] queue fill, [2..3] flush base
	float *qval = (float *)(qctl + 16);                                 // [CL_QCAP] coarse value of every queued candidate (round 5: the final-bound filter's input)

	const int tid = threadIdx.x, lane = tid & 63;
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int hq = lane >> 4, c = lane & 15;
	int split, qb;
	if (a.xcd_map) {
		const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
		split = (idx / a.nqb) * 8 + xcd;
		qb = idx % a.nqb;
	} else {
		split = blockIdx.x / a.nqb;
		qb = blockIdx.x % a.nqb;
	}
	const long long r_begin = a.row_first + (long long)split * a.split_rows;
	long long r_end = r_begin + a.split_rows;
	if (r_end > a.n)
		r_end = a.n;
	const int nblocks = r_end > r_begin ? (int)((r_end - r_begin + RT - 1) / RT) : 0;
	if (tid == 0)
		qctl[0] = 0u;
	const int qw = qb * QB + wave * QW;

	// B fragments, resident for the whole scan: fragment f = cb * KBT + kb lives in an AGPR quad when f >= NV (the last NAG
	// = 60 fragments: 240 of the 256 AGPRs), in VGPRs otherwise (36 fragments = 144 VGPRs)
	constexpr int NAG = KSPL == 2 ? 64 : 60, NV = NCB * KT - NAG; // (two parts: all 256 AGPRs -- with 16 left over hipcc parked a VGPR fragment there and copied it back in front of its MFMAs)
	static_assert(NV > 0 && NV * 4 <= 160, "VGPR-resident fragments");
	bf16x8 bqv[NV], bqa[NAG];
	{
		const bf16x8 *qsrc = (const bf16x8 *)a.qf;
#pragma unroll
		for (int cb = 0; cb < NCB; ++cb) {
			const size_t qblk16 = (size_t)qb * (QB / 16) + wave * NCB + cb;
#pragma unroll
			for (int kb = 0; kb < KT; ++kb) {
				const int f = cb * KT + kb;
				const bf16x8 t = qsrc[(qblk16 * KT + kb) * 64 + lane];
				if (f < NV) {
					bqv[f] = t;
				} else {
					bqa[f - NV] = t;
					asm volatile("" : "+a"(bqa[f - NV])); // into its AGPR quad now; every later use asks for "a"
				}
			}
		}
	}

	// LDS-DMA (as flat_collect_wide.hip): instruction inst = 4 i + wave fills LDS bytes [1024 inst, +1024) of the stage; lane l owns
	// 16-byte slot S = 64 inst + l = (row r = S / C, position p = S % C) and fetches chunk (p & ~15) | ((p & 15) ^ (r & 15))
	// (u: staged block = row block u / KSPL, part u % KSPL)
	auto dma_one = [&](int u, int stg, int i) {
		const char *base = (const char *)a.yb + (size_t)(r_begin + (long long)(u / KSPL) * RT) * GPITCH + (size_t)(u % KSPL) * PITCH; // uniform
		const int inst = 4 * i + wave;
		const int S = 64 * inst + lane, r = S / C, p = S - r * C;
		const unsigned off = (unsigned)(r * GPITCH + (((p & ~15) | ((p & 15) ^ (r & 15))) * 16));
		__builtin_amdgcn_global_load_lds((glb_f32c *)(base + off), (lds_f32c *)(smem + (stg * STAGE_BYTES + inst * 1024) / 4), 16, 0, 0);
	};
	auto dma_beta = [&](int u, int stg) { // wave 0 only
		const float *bb = a.yn + (r_begin + (long long)(u / KSPL) * RT); // uniform
		__builtin_amdgcn_global_load_lds((glb_f32c *)(bb + lane), (lds_f32c *)(smem + (NST * STAGE_BYTES) / 4 + stg * 64), 4, 0, 0);
	};
	if (nblocks > 0) {
#pragma unroll
		for (int b = 0; b < NST - 1; ++b) {
#pragma unroll
			for (int i = 0; i < DMA_PER_WAVE; ++i)
				dma_one(b, b, i);
			if (wave == 0)
				dma_beta(b, b);
		}
	}
	__syncthreads();

	const unsigned rbase = (unsigned)(c * PITCH) + (unsigned)(((hq ^ c) & 15) * 16);
	const unsigned qcnt_lds = (unsigned)(uintptr_t)((__attribute__((address_space(3))) unsigned *)qctl);
	const unsigned qbuf_lds = (unsigned)(uintptr_t)((__attribute__((address_space(3))) unsigned long long *)qbuf);
	const unsigned qval_lds = (unsigned)(uintptr_t)((__attribute__((address_space(3))) float *)qval);
	const unsigned cq_lds = (unsigned)(uintptr_t)((__attribute__((address_space(3))) float *)cqtab) + (unsigned)((wave * 16 + c) * 16);

	// candidates of one tile: rows whose coarse value reaches the pass bound of their query
	auto rare = [&](const f32x4b (&sv)[NCB], f32x4n cqv, long long row0, int nvalid) {
		int qo = qw;
		MVS_OPAQUE_VGPR(qo); // (keeps the per-query addresses of this path out of the hot loop's registers)
#pragma unroll
		for (int i = 0; i < NCB; ++i) {
			const int q = qo + 16 * i + c;
			const float c0 = cqv[i];
			unsigned m = 0u;
#pragma unroll
			for (int r = 0; r < 4; ++r)
				if (4 * hq + r < nvalid && sv[i][r] >= c0) // NaN on either side: false
					m |= 1u << r;
			if (a.rowmask && m != 0u) { // IDSelector: rejected rows are neither candidates nor evidence for the bound
				const unsigned long long rr = (unsigned long long)(row0 + 4 * hq);
				m &= (unsigned)(((const unsigned *)a.rowmask)[rr >> 5] >> (rr & 31u));
			}
			while (m != 0u) {
				const int j = __builtin_ctz(m);
				m &= m - 1u;
				const float lo = (j & 1) ? sv[i][1] : sv[i][0];
				const float hi = (j & 1) ? sv[i][3] : sv[i][2];
				const float v = (j & 2) ? hi : lo;
				const unsigned row = (unsigned)(row0 + 4 * hq + j);
				typedef __attribute__((address_space(1))) unsigned *GU;
				__hip_atomic_fetch_min((GU)(a.gslot + (size_t)q * NC) + (row & (unsigned)(NC - 1)), skey(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if (COLLECT) {
					unsigned pos;
					const unsigned one = 1u;
					asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&v"(pos) : "v"(qcnt_lds), "v"(one) : "memory");
					const unsigned long long ent = ((unsigned long long)(unsigned)q << 32) | row;
					if (pos < (unsigned)CL_QCAP) {
						asm volatile("ds_write_b64 %0, %1\n\tds_write_b32 %2, %3" ::"v"(qbuf_lds + 8u * pos), "v"(ent), "v"(qval_lds + 4u * pos), "v"(v) : "memory");
					} else { // a burst beyond the queue: straight to the stream (by hand, wait included: flat_collect.hip)
						unsigned long long gp;
						const unsigned long long one64 = 1ull;
						typedef __attribute__((address_space(1))) unsigned long long *GUL;
						asm volatile("global_atomic_add_x2 %0, %1, %2, off sc0\n\ts_waitcnt vmcnt(0)"
						             : "=&v"(gp)
						             : "v"((GUL)a.stream_cnt), "v"(one64)
						             : "memory");
						if ((long long)gp < a.stream_cap) {
							*((GUL)a.stream + gp) = ent;
							if (a.stream_s)
								a.stream_s[gp] = v;
						}
					}
				}
			}
		}
		// the slot / stream updates are done before the next LDS-DMA is issued: the tile barrier's vmcnt counts loads only
		asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
	};

	// bound refresh: lane (hq, c), hq < NCB, owns query c of column block hq; B = the kk-th best of its 16 class bests
	auto refresh = [&]() {
		if (hq < NCB) {
			int qo = qw;
			MVS_OPAQUE_VGPR(qo);
			const int q = qo + 16 * hq + c;
			const int qc = q < a.nq ? q : 0;
			if (a.pbnd != nullptr && (a.flags & CL_FROZEN)) { // lists beyond 128 entries: frozen bounds, one per query (csrc/flat_collect.hip)
				cqtab[(wave * 16 + c) * 4 + hq] = q < a.nq ? a.pbnd[qc] : __uint_as_float(0x7fc00000u);
				return;
			}
			const float e2v = __builtin_nontemporal_load(a.e2 + qc);
			// NC = 128 (32 < kk <= 128, round 6): four SUBSETS of 32 classes (class = row & 127, subset = class >> 5); the worst of the
			// subsets' ceil(kk / 4)-th best class values has >= kk distinct rows at least as good (csrc/flat_collect.hip)
			constexpr int SUBN = NC > 32 ? 32 : NC, NSUB = NC / SUBN;
			const int rank = NSUB == 1 ? a.nclass - 1 : (a.nclass + NSUB - 1) / NSUB - 1;
			unsigned kth = 0u;
#pragma unroll 1
			for (int sb = 0; sb < NSUB; ++sb) {
				const unsigned long long *src = (const unsigned long long *)(a.gslot + (size_t)qc * NC + sb * SUBN);
				unsigned long long w[SUBN / 2];
#pragma unroll
				for (int j = 0; j < SUBN / 2; ++j)
					w[j] = __hip_atomic_load(src + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
				for (int j = 0; j < SUBN / 2; ++j)
					asm volatile("" : "+v"(w[j]));
				unsigned key[SUBN];
#pragma unroll
				for (int j = 0; j < SUBN / 2; ++j) {
					key[2 * j] = (unsigned)w[j];
					key[2 * j + 1] = (unsigned)(w[j] >> 32);
				}
#pragma unroll
				for (int kbit = 2; kbit <= SUBN; kbit <<= 1)
#pragma unroll
					for (int jb = kbit >> 1; jb > 0; jb >>= 1)
#pragma unroll
						for (int x0 = 0; x0 < SUBN; ++x0) {
							const int x1 = x0 ^ jb;
							if (x1 > x0) {
								const unsigned lo = key[x0] < key[x1] ? key[x0] : key[x1];
								const unsigned hi = key[x0] < key[x1] ? key[x1] : key[x0];
								const bool asc = (x0 & kbit) == 0;
								key[x0] = asc ? lo : hi;
								key[x1] = asc ? hi : lo;
							}
						}
				unsigned ks = key[0];
#pragma unroll
				for (int j = 1; j < SUBN; ++j)
					ks = (rank == j) ? key[j] : ks;
				kth = ks > kth ? ks : kth; // (keys: smaller = better; the worst subset decides)
			}
			const unsigned neutral = skey(-FLT_MAX);
			const float B = skey2f(kth < neutral ? kth : neutral); // -FLT_MAX while fewer than kk classes are set
			// (2E = NaN stays NaN; NaN: nothing passes)
			cqtab[(wave * 16 + c) * 4 + hq] = q < a.nq ? B - e2v : __uint_as_float(0x7fc00000u);
		}
	};

	f32x4b acc[2][NCB]; // two accumulator sets: tile u lives in acc[u & 1] while tile u - 1 (the other set) is tested
	f32x4n pcq = {0.f, 0.f, 0.f, 0.f}; // the bounds tile u - 1 was scanned under
	bf16x8 A[RING];                    // A fragments: k-block kb of the current tile in A[kb % RING], read RA k-blocks ahead -- across tiles
	f32x4n Yv[2];                      // beta of the tile's rows, by tile parity
	int stg = 0;                       // stage of tile u = u % NST
	// A fragment (k-block kb) of a staged tile: byte c * PITCH + 256 (kb >> 2) + (rb16 ^ (64 (kb & 3)))
	auto read_a = [&](bf16x8 &dst, int stage, int kb) {
		const unsigned tb = (unsigned)(uintptr_t)((lds_f32c *)(smem + (stage * STAGE_BYTES) / 4)) + rbase;
		asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"((tb ^ (unsigned)((kb & 3) * 64)) + (unsigned)((kb >> 2) * 256)) : "memory");
	};
	auto read_y = [&](f32x4n &dst, int stage) {
		const unsigned nb_lds = (unsigned)(uintptr_t)((lds_f32c *)(nbuf + stage * 64 + 4 * hq));
		asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(nb_lds) : "memory");
	};
	static_assert(RA == 4, "the end-of-tile wait names A[0..3]");
	if (nblocks > 0) { // tile 0's beta and first fragments
		read_y(Yv[0], 0);
#pragma unroll
		for (int kb = 0; kb < RA; ++kb)
			read_a(A[kb], 0, kb);
		asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]), "+v"(Yv[0]));
	}
	// one tile; PAR = u & 1 as a compile-time constant (the accumulator sets must be registers, not an indexed array)
	// (hc: the part of the row block, compile time; v = u * KSPL + part is the staged block)
	auto tile = [&](auto parc, auto hc, const int u) {
		constexpr int par = decltype(parc)::value;
		constexpr int part = decltype(hc)::value;
		constexpr bool first = part == 0, last = part == KSPL - 1;
		const int v = u * KSPL + part;
		const int period = u < 8 ? 1 : (u < 64 ? 8 : (u < 512 ? 32 : 128));
		if (first && (u % period) == 0)
			refresh();
		const int nstg = stg + 1 == NST ? 0 : stg + 1, dstg = stg == 0 ? NST - 1 : stg - 1; // tile u + 1's stage; block u + NST - 1 goes where tile u - 1 was
		f32x4n cqv = pcq; // (read from the table in the first part; the later parts leave pcq alone)
		bool any_prev = false;
#pragma unroll
		for (int kb = 0; kb < KBT; ++kb) {
			if (kb == KB_BAR) {
				// block u + 1 has landed for every wave (the newest block -- u + 2, this wave's last DMA_PER_WAVE (+ 1: beta) loads,
				// nothing else is in flight, loads return in order -- stays in flight); everybody is done with tile u - 1's stage
				// (NST - 3 newer blocks stay in flight: u + 2 .. u + NST - 2)
				if (wave == 0)
					asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NST - 3) * (DMA_PER_WAVE + 1)) : "memory");
				else
					asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NST - 3) * DMA_PER_WAVE) : "memory");
			}
			// Round 5: a lone wave issues IN ORDER -- whatever stands between two groups of MFMAs waits for the matrix pipe to take the
			// group's last MFMA and then runs with only that one's 16 cycles to hide under (rounds 3-4: fragment read, wait, LDS-DMA
			// address + issue, bound read all sat behind the k-block's NCB MFMAs: the pipe was 52 % busy, profiles/r5_pmc_c4.txt).
			// Now ONE such instruction group follows EACH MFMA of the k-block: it issues while that MFMA runs and the next MFMA could
			// not have issued anyway.  Fragment kb must have arrived before the k-block's first MFMA: LDS returns in order and
			// the reads of fragments kb + 1 .. kb + RA - 1 are younger (the read of kb + RA is issued behind this k-block's first MFMA).
			asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(A[kb % RING]), "+v"(Yv[par]), "+v"(cqv), "+v"(A[(kb + 1) % RING]) : "n"(RA - 1));
#pragma unroll
			for (int i = 0; i < NCB; ++i) {
				const int f = i * KT + part * KBT + kb;
				const bool start = first && kb == 0; // the chain starts at beta(row) in the row block's first part
				// A column block is accumulated EITHER by the builtin (all its fragments in VGPRs) OR by hand-written MFMAs
				// (any of them in AGPRs): mixing the two on one accumulator made the compiler copy it between the files with
				// v_accvgpr_read right in front of a hand-written MFMA -- a VALU write -> MFMA srcC hazard nobody pads.
				const bool by_hand = (i + 1) * KT > NV;
				if (!by_hand) {
					if (start) // s comes out of the matrix pipe
						acc[par][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[kb % RING], bqv[f < NV ? f : 0], Yv[par], 0, 0, 0);
					else
						acc[par][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[kb % RING], bqv[f < NV ? f : 0], acc[par][i], 0, 0, 0);
				} else if (f < NV) { // srcB in VGPRs
					if (start)
						asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %3"
						             : "=&v"(acc[par][i])
						             : "v"(A[kb % RING]), "v"(bqv[f < NV ? f : 0]), "v"(Yv[par]));
					else
						asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0"
						             : "+v"(acc[par][i])
						             : "v"(A[kb % RING]), "v"(bqv[f < NV ? f : 0]));
				} else { // srcB from an AGPR quad
					if (start)
						asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %3"
						             : "=&v"(acc[par][i])
						             : "v"(A[kb % RING]), "a"(bqa[f >= NV ? f - NV : 0]), "v"(Yv[par]));
					else
						asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0"
						             : "+v"(acc[par][i])
						             : "v"(A[kb % RING]), "a"(bqa[f >= NV ? f - NV : 0]));
				}
				__builtin_amdgcn_sched_barrier(0);
				// ... and behind MFMA i, ONE of the k-block's other duties:
				if (i == 0) { // the fragment RA k-blocks ahead (its ring slot was consumed RING - RA k-blocks ago)
					if (kb + RA < KBT)
						read_a(A[(kb + RA) % RING], stg, kb + RA);
					else
						read_a(A[(kb + RA) % RING], nstg, kb + RA - KBT); // the next tile's first fragments (its block landed at the barrier)
				}
				if (i == (NCB > 2 ? 1 : NCB - 1)) { // the staging of block u + 3, this tile's bounds, the next block's beta
					if (kb > KB_BAR && ((kb - KB_BAR) & 1) && (kb - KB_BAR) / 2 < DMA_PER_WAVE)
						dma_one(v + NST - 1, dstg, (kb - KB_BAR) / 2); // one LDS-DMA instruction per two k-blocks
					if (kb == KB_BAR + 2 && wave == 0)
						dma_beta(v + NST - 1, dstg);
					if (first && kb == 2)
						asm volatile("ds_read_b128 %0, %1" : "=v"(cqv) : "v"(cq_lds) : "memory"); // this tile's bounds (tested one tile later)
					if (kb == KBT - RA) // (beta of the staged block behind this one: the next row block's when this is the last part)
						read_y(Yv[par ^ 1], nstg); // (not the last part: block v + 1 carries this row block's beta again -- unused, reloaded at the last part)
				}
				if (i == (NCB > 2 ? 2 : NCB - 1) && first && kb == 1 && u > 0) { // tile u - 1's running maxima against its bounds
#pragma unroll
					for (int i3 = 0; i3 < NCB; ++i3) {
						const f32x4b &sv = acc[par ^ 1][i3];
						const float mx = __builtin_fmaxf(__builtin_fmaxf(sv[0], sv[1]), __builtin_fmaxf(sv[2], sv[3]));
						any_prev = any_prev || (mx >= pcq[i3]);
					}
				}
				__builtin_amdgcn_sched_barrier(0);
			}
		}
		// The fragments (and beta) read ahead for the next tile must have LANDED before control leaves this straight-line block:
		// hipcc counts an asm load's destination as written at the end of the statement and is free to copy or spill it on the
		// way through the branches below (rare path, flush, bound refresh) -- a copy of a register whose ds_read is still in
		// flight is garbage.  The last RA k-blocks' MFMAs are queued behind this wait, so it costs nothing.
		asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]), "+v"(Yv[par ^ 1]), "+v"(cqv));
		if (first && u > 0 && __builtin_amdgcn_ballot_w64(any_prev) != 0ull) {
			const long long prow0 = r_begin + (long long)(u - 1) * RT;
			const int pnvalid = (int)((r_end - prow0) < RT ? (r_end - prow0) : RT);
			rare(acc[par ^ 1], pcq, prow0, pnvalid);
		}
		pcq = cqv;
		stg = nstg;
		if (COLLECT && last && (u % FLUSH_EVERY) == FLUSH_EVERY - 1 && u != nblocks - 1) {
			// (the fragments read ahead for the next tile are in registers; the compiled LDS accesses below make hipcc drain the
			// LDS-DMA in flight first -- once per FLUSH_EVERY tiles)
			__syncthreads(); // the tile's own barrier stands in mid-tile: every wave's appends of this tile must be in before the look
			const unsigned fill = qctl[0];
			__syncthreads(); // everybody has read the same fill before anyone appends again
			const unsigned n = fill < (unsigned)CL_QCAP ? fill : (unsigned)CL_QCAP;
			if (n >= (unsigned)CL_QCAP / 2) {
				if (tid == 0) {
					*(unsigned long long *)(qctl + 2) = atomicAdd(a.stream_cnt, (unsigned long long)n);
					qctl[0] = 0u;
				}
				__syncthreads();
				const unsigned long long base = *(const unsigned long long *)(qctl + 2);
				for (unsigned i = tid; i < n; i += 256)
					if ((long long)(base + i) < a.stream_cap) {
						a.stream[base + i] = qbuf[i];
						if (a.stream_s)
							a.stream_s[base + i] = qval[i];
					}
				__syncthreads();
			}
		}
	};
	for (int u0 = 0; u0 < nblocks; u0 += 2) {
		tile(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, u0);
		if (KSPL > 1)
			tile(std::integral_constant<int, 0>{}, std::integral_constant<int, KSPL - 1>{}, u0);
		if (u0 + 1 < nblocks) {
			tile(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, u0 + 1);
			if (KSPL > 1)
				tile(std::integral_constant<int, 1>{}, std::integral_constant<int, KSPL - 1>{}, u0 + 1);
		}
	}
	asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); // (the blocks fetched and the fragments read past the split's end)
	// (the hand-written MFMAs have drained before the vector ALU reads their accumulators: >= 19 wait states on gfx950)
	asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
	auto last_tile = [&](auto parc) { // the last tile's test (its accumulator set as a compile-time constant)
		constexpr int lp = decltype(parc)::value;
		bool any_t = false;
#pragma unroll
		for (int i = 0; i < NCB; ++i) {
			const f32x4b &sv = acc[lp][i];
			const float mx = __builtin_fmaxf(__builtin_fmaxf(sv[0], sv[1]), __builtin_fmaxf(sv[2], sv[3]));
			any_t = any_t || (mx >= pcq[i]);
		}
		if (__builtin_amdgcn_ballot_w64(any_t) != 0ull) {
			const long long prow0 = r_begin + (long long)(nblocks - 1) * RT;
			const int pnvalid = (int)((r_end - prow0) < RT ? (r_end - prow0) : RT);
			rare(acc[lp], pcq, prow0, pnvalid);
		}
	};
	if (nblocks > 0) {
		if ((nblocks - 1) & 1)
			last_tile(std::integral_constant<int, 1>{});
		else
			last_tile(std::integral_constant<int, 0>{});
	}
	if (COLLECT) {
		__syncthreads(); // every wave's appends are in
		const unsigned fill = qctl[0];
		const unsigned n = fill < (unsigned)CL_QCAP ? fill : (unsigned)CL_QCAP;
		if (n > 0) {
			if (tid == 0)
				*(unsigned long long *)(qctl + 2) = atomicAdd(a.stream_cnt, (unsigned long long)n);
			__syncthreads();
			const unsigned long long base = *(const unsigned long long *)(qctl + 2);
			for (unsigned i = tid; i < n; i += 256)
				if ((long long)(base + i) < a.stream_cap) {
					a.stream[base + i] = qbuf[i];
					if (a.stream_s)
						a.stream_s[base + i] = qval[i];
				}
		}
	}
}

int collect_big_ncb(int dp1) {
	return dp1 == 768 ? 4 : (dp1 == 1024 ? 3 : 2); // (1536: 2 x 48 k-blocks = the 96 fragments of 4 x 24)
}
int collect_big_qblock(int dp1) {
	return 4 * 16 * collect_big_ncb(dp1);
}
size_t collect_big_lds_bytes(int dp1) {
	const int part = dp1 == 1536 ? 768 : dp1; // dims of a staged block (the 1536-dim store is staged in two parts per row block)
	return (size_t)big_stages(16 * part * 2) * (16 * part * 2 + 64 * 4) + (size_t)CL_QCAP * 8 + 4 * 16 * 4 * 4 + 64 + (size_t)CL_QCAP * 4;
}

template <int KBT, int NCB, int KSPL = 1>
static void launch_big_inst(int metric, bool collect, const CollectArgs &a, int grid, size_t lds, hipStream_t st) {
#define MVS_BIG(L2, CO, NCV)                                                                                      \
	{                                                                                                             \
		auto kern = flat_bf16_big_kernel<KBT, NCB, L2, CO, KSPL, NCV>;                                            \
		ensure_dynamic_lds((const void *)kern, lds);                                                              \
		hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, st, a);                                    \
	}
#define MVS_BIG_NC(NCV)                                                                                           \
	{                                                                                                             \
		if (metric == METRIC_L2 && collect)                                                                       \
			MVS_BIG(true, true, NCV)                                                                              \
		else if (metric == METRIC_L2)                                                                             \
			MVS_BIG(true, false, NCV)                                                                             \
		else if (collect)                                                                                         \
			MVS_BIG(false, true, NCV)                                                                             \
		else                                                                                                      \
			MVS_BIG(false, false, NCV)                                                                            \
	}
	if (a.slot_stride == 128) // 32 < kk <= 128: four subsets of 32 row classes (round 6)
		MVS_BIG_NC(128)
	else if (a.slot_stride == 32) // 16 < kk <= 32: 32 row classes per query
		MVS_BIG_NC(32)
	else
		MVS_BIG_NC(16)
#undef MVS_BIG_NC
#undef MVS_BIG
	MVS_HIP(hipGetLastError());
}

void launch_collect_big(int dp1, int metric, bool collect, const CollectArgs &a, int grid, hipStream_t st) {
	const size_t lds = collect_big_lds_bytes(dp1);
	if (dp1 == 768)
		launch_big_inst<24, 4>(metric, collect, a, grid, lds, st);
	else if (dp1 == 1024)
		launch_big_inst<32, 3>(metric, collect, a, grid, lds, st);
	else if (dp1 == 1536)
		launch_big_inst<24, 2, 2>(metric, collect, a, grid, lds, st);
	else
		throw_faiss("mvs::launch_collect_big", __FILE__, "no instance for a %d-dim store", dp1);
}

} // namespace mvs
