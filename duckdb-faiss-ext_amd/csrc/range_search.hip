// csrc/range_search.hip -- faiss::Index::range_search on the device: every row within a fixed radius of each query, a
// variable-length result (lims, distances, labels) where search keeps a k-list.  The contract is the "range search" block of
// include/mi355_faiss.h and DESIGN.md 3.11.
//
// Replaces what a FAISS host reaches through index->range_search(n, x, radius, result, params)
//   -> IndexFlat::range_search -> range_search_L2sqr / range_search_inner_product (RangeSearchBlockResultHandler)
//   -> IndexIVF::range_search -> range_search_preassigned (IVFFlatScanner::scan_codes_range)
// [UPSTREAM FAISS, restated from memory: strict dis < radius (L2) / dis > radius (inner product)].
//
// Two scans, one emission scheme, one grouping stage:
//   range_pair_kernel  (VALU, exact)   thread <-> database row, 256-row tiles staged through LDS in chunks of KC columns; up to
//                      RQ queries per work item, read with wave-uniform (scalar) loads.  The per-pair chains of
//                      csrc/flat_direct.hip, plus the FORMULA mode for L2 -- ip as the k-ordered chain, (xn + yn) - 2 ip in two
//                      roundings, clamped at 0: the BLAS-branch value.  Grid mode (Flat) or item mode (IVF lists).
//   range_mfma_kernel  (f32 MFMA 32x32x2, dp <= 128)   the BLAS-branch value on the matrix pipe: 64-row tiles in two LDS buffers (the
//                      next tile is staged piece by piece behind the current tile's MFMAs), the wave's 32 queries resident as B
//                      fragments (query on the lane, as in csrc/flat_mfma.hip), the same epilogue arithmetic.
//   emission           an entry is key = query << 32 | ordinal and payload = distance bits << 32 | position in the row store.  One
//                      wave-aggregated atomicAdd on the global cursor per wave and tile (ballot / prefix, one atomic by the first lane);
//                      entries past the capacity are COUNTED but not written, so that the host learns the exact size and scans once more.
//   grouping           rocprim radix sort of the (key, payload) pairs by key; lims[q] = lower bound of q << 32 (one thread per query);
//                      a small kernel writes distances and labels.
#include "index.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

namespace mvs {

namespace {

constexpr int RTILE = 256; // rows of a VALU tile = threads of a workgroup
constexpr int RQ = 16;     // query slots of a VALU work item

struct RangeArgs {
	const float *xq; // [nq][dp] the chunk's queries, zero padded to dp
	const float *xn; // [nq] squared norms (formula mode / MFMA kernel, L2)
	const float *yb; // row store [n][dp]
	const float *yn; // [n] squared row norms (formula mode / MFMA kernel, L2)
	long long n, split_rows;
	int nq, dp, interleaved, formula, ngroups;
	float radius;
	SelectorDev sel;
	const long long *idmap;  // selector tests idmap[stored id] (IndexIDMap: the external id)
	const long long *rowids; // stored id of a row (IVF); null: the row number
	// item mode (IVF): {row_begin, row_end, qoff, nq_item} as in csrc/ivf_scan.hip; slot s of an item is query qidx[qoff + s] and its
	// ordinals start at obase[qoff + s] (the rows the query's earlier probes hold)
	const int4 *items;
	const int *qidx;
	const unsigned *obase;
	unsigned long long *keys, *vals, *cnt;
	long long cap;
};

__device__ __forceinline__ bool range_sel_member(const SelectorDev &s, long long id) {
	if (s.kind == MVS_SEL_BITMAP) {
		const unsigned long long u = (unsigned long long)id;
		if ((u >> 3) >= (unsigned long long)s.nbytes)
			return false;
		return (s.bitmap[u >> 3] >> (u & 7)) & 1;
	}
	if (s.kind == MVS_SEL_BATCH) {
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
	return true;
}

// both comparisons are false for a NaN distance and for a NaN radius
template <bool IS_L2>
__device__ __forceinline__ bool range_hit(float v, float radius) {
	return IS_L2 ? v < radius : v > radius;
}

// the lane's `mine` entries go to stream slots [base, base + mine): ONE atomicAdd per wave
__device__ __forceinline__ long long range_reserve(int mine, unsigned long long *cnt) {
	const int lane = threadIdx.x & 63;
	int incl = mine;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const int o = __shfl_up(incl, off);
		if (lane >= off)
			incl += o;
	}
	const int total = __shfl(incl, 63);
	unsigned long long base = 0;
	if (lane == 0)
		base = atomicAdd(cnt, (unsigned long long)total);
	base = __shfl(base, 0);
	return (long long)base + (incl - mine);
}

template <bool IS_L2, int KC>
__global__ __launch_bounds__(RTILE) void range_pair_kernel(const RangeArgs a) {
	constexpr int LDA = KC + 1;
	constexpr int F4_PER_ROW = KC / 4, NLD = F4_PER_ROW; // 256 * KC / 4 float4 per chunk, 256 threads
	__shared__ float tbuf[RTILE * LDA];
	const int tid = threadIdx.x;
	long long r_begin, r_end;
	int q0 = 0, qbase = 0, nq_item;
	if (a.items) {
		const int4 it = a.items[blockIdx.x];
		r_begin = it.x;
		r_end = it.y;
		qbase = it.z;
		nq_item = it.w;
	} else {
		const int split = blockIdx.x / a.ngroups;
		q0 = (blockIdx.x % a.ngroups) * RQ;
		r_begin = (long long)split * a.split_rows;
		r_end = r_begin + a.split_rows;
		nq_item = a.nq - q0 < RQ ? a.nq - q0 : RQ;
	}
	if (r_end > a.n)
		r_end = a.n;
	if (nq_item <= 0 || r_end <= r_begin) // (the whole workgroup, before any barrier)
		return;
	// query number of slot qq (wave-uniform); unused slots read the item's first query and are never recorded
	auto qnum = [&](int qq) -> int {
		const int s = qq < nq_item ? qq : 0;
		return a.items ? __builtin_amdgcn_readfirstlane(a.qidx[qbase + s]) : q0 + s;
	};
	const int ntiles = (int)((r_end - r_begin + RTILE - 1) / RTILE);
	const int nch = a.dp / KC;
	for (int tile = 0; tile < ntiles; ++tile) {
		const long long row0 = r_begin + (long long)tile * RTILE;
		float acc[RQ];
#pragma unroll
		for (int qq = 0; qq < RQ; ++qq)
			acc[qq] = 0.f;
		for (int ch = 0; ch < nch; ++ch) {
			__syncthreads(); // the previous chunk's readers are done
#pragma unroll
			for (int i = 0; i < NLD; ++i) {
				const int f = i * RTILE + tid;
				const int row = f / F4_PER_ROW, c4 = f - row * F4_PER_ROW;
				long long gr = row0 + row;
				if (gr >= r_end)
					gr = r_end - 1;
				const float4 s = *(const float4 *)(a.yb + (size_t)gr * a.dp + ch * KC + c4 * 4);
				float *p = tbuf + row * LDA + c4 * 4;
				// back to natural k order (FlatGeom::pair_interleaved: the layout follows bit 4 of the row's index in the store)
				if (!a.interleaved) {
					p[0] = s.x, p[1] = s.y, p[2] = s.z, p[3] = s.w;
				} else if (gr & 16) { // stored [k1,k3,k0,k2]
					p[0] = s.z, p[1] = s.x, p[2] = s.w, p[3] = s.y;
				} else { // stored [k0,k2,k1,k3]
					p[0] = s.x, p[1] = s.z, p[2] = s.y, p[3] = s.w;
				}
			}
			__syncthreads();
			float y[KC];
#pragma unroll
			for (int kk = 0; kk < KC; ++kk)
				y[kk] = tbuf[tid * LDA + kk];
#pragma unroll
			for (int qq = 0; qq < RQ; ++qq) {
				if (qq >= nq_item) // (wave-uniform; no break: the loop must unroll for acc[] to stay in registers)
					continue;
				// wave-uniform address in the constant address space => scalar loads
				typedef __attribute__((address_space(4))) const float cfloat;
				cfloat *xs = (cfloat *)(a.xq + (size_t)qnum(qq) * a.dp + ch * KC);
				float s = acc[qq];
#pragma unroll
				for (int kk = 0; kk < KC; ++kk) {
					if (IS_L2 && !a.formula) {
						const float t = xs[kk] - y[kk];
						s = fmaf(t, t, s);
					} else {
						s = fmaf(xs[kk], y[kk], s);
					}
				}
				acc[qq] = s;
			}
		}
		const long long row = row0 + tid;
		bool valid = row < r_end;
		if (valid && a.sel.kind != MVS_SEL_NONE) {
			const long long lab = a.rowids ? a.rowids[row] : row;
			valid = range_sel_member(a.sel, a.idmap ? a.idmap[lab] : lab);
		}
		float ynr = 0.f;
		if (IS_L2 && a.formula)
			ynr = a.yn[row < r_end ? row : r_end - 1];
		unsigned hits = 0; // bit qq: this row is a hit of slot qq
#pragma unroll
		for (int qq = 0; qq < RQ; ++qq) {
			if (qq >= nq_item)
				continue;
			float v = acc[qq];
			if (IS_L2 && a.formula) {
				v = fmaf(-2.0f, v, a.xn[qnum(qq)] + ynr); // (xn + yn) - 2 ip, two roundings as the oracle
				v = v < 0.f ? 0.f : v;
				acc[qq] = v;
			}
			if (valid && range_hit<IS_L2>(v, a.radius))
				hits |= 1u << qq;
		}
		if (__builtin_amdgcn_ballot_w64(hits != 0u) == 0ull)
			continue;
		long long pos = range_reserve(__popc(hits), a.cnt);
#pragma unroll
		for (int qq = 0; qq < RQ; ++qq) {
			if (!((hits >> qq) & 1u))
				continue;
			if (pos < a.cap) {
				const unsigned ord = a.items ? a.obase[qbase + qq] + (unsigned)(row - r_begin) : (unsigned)row;
				a.keys[pos] = ((unsigned long long)(unsigned)qnum(qq) << 32) | ord;
				a.vals[pos] = ((unsigned long long)__float_as_uint(acc[qq]) << 32) | (unsigned)row;
			}
			++pos;
		}
	}
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Flat, BLAS branch, dp = 2 KSTEPS <= 128.  Workgroup = 4 waves x 32 queries; D[i][j] of v_mfma_f32_32x32x2_f32 lands with the query
// j = lane & 31 on the lane and row i = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) in the accumulator registers.  The instruction is a
// k-ordered fma chain (csrc/flat_mfma.hip, "arithmetic contract"): k-step s multiplies column 2 s + (lane >> 5).
template <bool IS_L2, int KSTEPS>
__global__ __launch_bounds__(256, 2) void range_mfma_kernel(const RangeArgs a) {
	constexpr int KC = 2 * KSTEPS, BN = 64, LDA = KC + 1;
	constexpr int F4_PER_ROW = KC / 4, NF4 = BN * F4_PER_ROW; // float4 pieces of a tile
	constexpr int NLD = (NF4 + 255) / 256;                    // ... per thread
	constexpr int SPG = KSTEPS / NLD;                         // k-steps of the MFMA loop between two staging pieces
	static_assert(KSTEPS % NLD == 0, "");
	// two tile buffers: piece g of the NEXT tile is loaded at the head of k-step group g and stored behind that group's MFMAs, so
	// one float4 per thread is in flight instead of the whole next tile (the d = 128 instance spilled with the latter)
	__shared__ float tbuf[2][BN * LDA];
	__shared__ float nbuf[2][BN];
	const int tid = threadIdx.x, lane = tid & 63;
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int h = lane >> 5, c = lane & 31;
	const int split = blockIdx.x / a.ngroups, qb = blockIdx.x % a.ngroups;
	const int q = qb * QBLOCK + wave * WAVE_Q + c;
	const bool qvalid = q < a.nq;
	long long r_begin = (long long)split * a.split_rows, r_end = r_begin + a.split_rows;
	if (r_end > a.n)
		r_end = a.n;
	if (r_end <= r_begin)
		return;
	const int ntiles = (int)((r_end - r_begin + BN - 1) / BN);
	// B fragments: the lane's query, columns 2 s + h (xq is zero padded to whole 128-query blocks)
	float qf[KSTEPS];
	const float *xr = a.xq + (size_t)q * KC + h;
#pragma unroll
	for (int s = 0; s < KSTEPS; ++s)
		qf[s] = xr[2 * s];
	const float xnq = (IS_L2 && qvalid) ? a.xn[q] : 0.f;

	// piece i of a tile: float4 number i * 256 + tid of its [64][KC] rows (rows past the end: the last row, masked in the epilogue)
	auto piece_load = [&](int tile, int i, float4 &v, long long &gr) {
		const int f = i * 256 + tid;
		const int row = f / F4_PER_ROW, c4 = f - row * F4_PER_ROW;
		gr = r_begin + (long long)tile * BN + row;
		if (gr >= r_end)
			gr = r_end - 1;
		if (NF4 % 256 == 0 || f < NF4)
			v = *(const float4 *)(a.yb + (size_t)gr * KC + c4 * 4);
	};
	auto piece_store = [&](int buf, int i, const float4 &s, long long gr) {
		const int f = i * 256 + tid;
		const int row = f / F4_PER_ROW, c4 = f - row * F4_PER_ROW;
		if (!(NF4 % 256 == 0 || f < NF4))
			return;
		float *p = tbuf[buf] + row * LDA + c4 * 4;
		// back to natural k order (FlatGeom::pair_interleaved: the layout follows bit 4 of the row's index in the store)
		if (!a.interleaved) {
			p[0] = s.x, p[1] = s.y, p[2] = s.z, p[3] = s.w;
		} else if (gr & 16) {
			p[0] = s.z, p[1] = s.x, p[2] = s.w, p[3] = s.y;
		} else {
			p[0] = s.x, p[1] = s.z, p[2] = s.y, p[3] = s.w;
		}
	};
	auto norms_stage = [&](int tile, int buf) {
		if (IS_L2 && tid < BN) {
			long long gr = r_begin + (long long)tile * BN + tid;
			if (gr >= r_end)
				gr = r_end - 1;
			nbuf[buf][tid] = a.yn[gr];
		}
	};

#pragma unroll
	for (int i = 0; i < NLD; ++i) {
		float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
		long long gr;
		piece_load(0, i, v, gr);
		piece_store(0, i, v, gr);
	}
	norms_stage(0, 0);
	__syncthreads();
	for (int tile = 0; tile < ntiles; ++tile) {
		const int buf = tile & 1;
		const bool more = tile + 1 < ntiles;
		f32x16 acc[2];
#pragma unroll
		for (int t = 0; t < 2; ++t)
#pragma unroll
			for (int r = 0; r < 16; ++r)
				acc[t][r] = 0.f;
		const float *A0 = tbuf[buf] + c * LDA + h, *A1 = tbuf[buf] + (32 + c) * LDA + h;
#pragma unroll
		for (int g = 0; g < NLD; ++g) {
			float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
			long long gr = 0;
			if (more)
				piece_load(tile + 1, g, v, gr);
#pragma unroll
			for (int s = g * SPG; s < (g + 1) * SPG; ++s) {
				acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[2 * s], qf[s], acc[0], 0, 0, 0);
				acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[2 * s], qf[s], acc[1], 0, 0, 0);
			}
			if (more)
				piece_store(buf ^ 1, g, v, gr); // (the other buffer: its readers finished before the barrier that ended the last tile)
		}
		if (more)
			norms_stage(tile + 1, buf ^ 1);
		const long long row0 = r_begin + (long long)tile * BN;
		unsigned hits = 0; // bit t * 16 + r
#pragma unroll
		for (int t = 0; t < 2; ++t)
#pragma unroll
			for (int r = 0; r < 16; ++r) {
				const int rl = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
				float v = acc[t][r];
				if (IS_L2) {
					v = fmaf(-2.0f, v, xnq + nbuf[buf][rl]); // (xn + yn) - 2 ip, two roundings as the oracle
					v = v < 0.f ? 0.f : v;
					acc[t][r] = v;
				}
				if (qvalid && row0 + rl < r_end && range_hit<IS_L2>(v, a.radius))
					hits |= 1u << (t * 16 + r);
			}
		if (__builtin_amdgcn_ballot_w64(hits != 0u) != 0ull) {
			long long pos = range_reserve(__popc(hits), a.cnt);
#pragma unroll
			for (int t = 0; t < 2; ++t)
#pragma unroll
				for (int r = 0; r < 16; ++r) {
					if (!((hits >> (t * 16 + r)) & 1u))
						continue;
					if (pos < a.cap) {
						const unsigned row = (unsigned)(row0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h);
						a.keys[pos] = ((unsigned long long)(unsigned)q << 32) | row;
						a.vals[pos] = ((unsigned long long)__float_as_uint(acc[t][r]) << 32) | row;
					}
					++pos;
				}
		}
		__syncthreads(); // the next tile is whole in the other buffer, and this buffer's readers are done
	}
}

// lims[q] = the first sorted entry whose query is >= q: one thread per query (and one for the end), a binary search
__global__ void range_lims_kernel(const unsigned long long *__restrict__ skeys, long long n, int nq, long long *__restrict__ lims) {
	const int q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q > nq)
		return;
	const unsigned long long key = (unsigned long long)(unsigned)q << 32;
	long long lo = 0, hi = n;
	while (lo < hi) {
		const long long mid = (lo + hi) >> 1;
		if (skeys[mid] < key)
			lo = mid + 1;
		else
			hi = mid;
	}
	lims[q] = lo;
}

__global__ void range_emit_kernel(const unsigned long long *__restrict__ svals, long long n, const long long *__restrict__ rowids,
                                  const long long *__restrict__ idmap, long long label_offset, float *__restrict__ D,
                                  long long *__restrict__ I) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const unsigned long long v = svals[i];
	D[i] = __uint_as_float((unsigned)(v >> 32));
	long long lab = (long long)(unsigned)v;
	if (rowids)
		lab = rowids[lab];
	I[i] = idmap ? idmap[lab] : lab + label_offset;
}

// one work item per (query, probe rank): the whole probed list, the query alone in its slot, ordinals behind the earlier probes' rows
__global__ void range_ivf_items_kernel(const long long *__restrict__ coarse, int nq, int np, const long long *__restrict__ list_off,
                                       int4 *__restrict__ items, int *__restrict__ qidx, unsigned *__restrict__ obase) {
	const int q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= nq)
		return;
	unsigned run = 0;
	for (int r = 0; r < np; ++r) {
		const long long l = coarse[(size_t)q * np + r];
		long long b = 0, e = 0;
		if (l >= 0) { // (-1: the quantiser had fewer than np answers)
			b = list_off[l];
			e = list_off[l + 1];
		}
		const size_t p = (size_t)q * np + r;
		items[p] = make_int4((int)b, (int)e, (int)p, e > b ? 1 : 0);
		qidx[p] = q;
		obase[p] = run;
		run += (unsigned)(e - b);
	}
}

template <bool IS_L2>
void launch_pair(const RangeArgs &a, int grid, hipStream_t st) {
	const int kc = a.dp < 32 ? a.dp : 32;
	if (kc == 8)
		hipLaunchKernelGGL((range_pair_kernel<IS_L2, 8>), dim3(grid), dim3(RTILE), 0, st, a);
	else if (kc == 16)
		hipLaunchKernelGGL((range_pair_kernel<IS_L2, 16>), dim3(grid), dim3(RTILE), 0, st, a);
	else
		hipLaunchKernelGGL((range_pair_kernel<IS_L2, 32>), dim3(grid), dim3(RTILE), 0, st, a);
	MVS_HIP(hipGetLastError());
}
template <bool IS_L2>
void launch_mfma(const RangeArgs &a, int grid, hipStream_t st) {
	switch (a.dp) {
	case 8:
		hipLaunchKernelGGL((range_mfma_kernel<IS_L2, 4>), dim3(grid), dim3(256), 0, st, a);
		break;
	case 16:
		hipLaunchKernelGGL((range_mfma_kernel<IS_L2, 8>), dim3(grid), dim3(256), 0, st, a);
		break;
	case 32:
		hipLaunchKernelGGL((range_mfma_kernel<IS_L2, 16>), dim3(grid), dim3(256), 0, st, a);
		break;
	case 64:
		hipLaunchKernelGGL((range_mfma_kernel<IS_L2, 32>), dim3(grid), dim3(256), 0, st, a);
		break;
	case 128:
		hipLaunchKernelGGL((range_mfma_kernel<IS_L2, 64>), dim3(grid), dim3(256), 0, st, a);
		break;
	default:
		throw_faiss("mvs::launch_range_mfma", __FILE__, "no instance for a row pitch of %d floats", a.dp);
	}
	MVS_HIP(hipGetLastError());
}

int range_qbits(int64_t nq) {
	int qbits = 1;
	while (((int64_t)1 << qbits) < nq + 1)
		++qbits;
	return qbits;
}

} // namespace

bool range_mfma_supported(const FlatGeom &g) {
	return g.dp <= 128 && (g.dp == 8 || g.dp == 16 || g.dp == 32 || g.dp == 64 || g.dp == 128);
}

void launch_range_flat(const RangeScan &s, bool mfma, int *grid_out, hipStream_t st) {
	RangeArgs a;
	memset(&a, 0, sizeof a);
	a.xq = s.xq, a.xn = s.xn, a.yb = s.rows, a.yn = s.norms;
	a.n = s.nrows, a.nq = (int)s.nq, a.dp = s.dp, a.interleaved = s.interleaved ? 1 : 0, a.formula = s.formula ? 1 : 0;
	a.radius = s.radius, a.sel = s.sel, a.idmap = (const long long *)s.idmap_sel;
	a.keys = s.keys, a.vals = s.vals, a.cnt = s.cnt, a.cap = s.cap;
	const bool l2 = s.metric == METRIC_L2;
	if (mfma) {
		// 64-row tiles; enough row splits to fill the device a few times over, each at least 16 tiles long where the rows allow it
		a.ngroups = (int)((s.nq + QBLOCK - 1) / QBLOCK);
		const int64_t ntiles = (s.nrows + 63) / 64;
		int64_t nsplit = std::max<int64_t>(1, std::min<int64_t>(4096 / a.ngroups, ntiles / 16));
		a.split_rows = (ntiles + nsplit - 1) / nsplit * 64;
		nsplit = (s.nrows + a.split_rows - 1) / a.split_rows;
		const int grid = (int)(nsplit * a.ngroups);
		l2 ? launch_mfma<true>(a, grid, st) : launch_mfma<false>(a, grid, st);
		*grid_out = grid;
		return;
	}
	a.ngroups = (int)((s.nq + RQ - 1) / RQ);
	const int64_t ntiles = (s.nrows + RTILE - 1) / RTILE;
	int64_t nsplit = std::max<int64_t>(1, std::min<int64_t>(4096 / a.ngroups, ntiles));
	a.split_rows = (ntiles + nsplit - 1) / nsplit * RTILE;
	nsplit = (s.nrows + a.split_rows - 1) / a.split_rows;
	const int grid = (int)(nsplit * a.ngroups);
	l2 ? launch_pair<true>(a, grid, st) : launch_pair<false>(a, grid, st);
	*grid_out = grid;
}

size_t range_ivf_item_bytes(int64_t npairs) {
	return (size_t)std::max<int64_t>(npairs, 1) * (sizeof(int4) + sizeof(int) + sizeof(unsigned));
}

void launch_range_ivf(const RangeScan &s, const int64_t *d_coarse, int np, const int64_t *d_list_off, const int64_t *d_rowids, void *d_items,
                      hipStream_t st) {
	const int64_t npairs = s.nq * np;
	if (npairs <= 0)
		return;
	int4 *items = (int4 *)d_items;
	int *qidx = (int *)(items + npairs);
	unsigned *obase = (unsigned *)(qidx + npairs);
	hipLaunchKernelGGL(range_ivf_items_kernel, dim3((unsigned)((s.nq + 255) / 256)), dim3(256), 0, st, (const long long *)d_coarse, (int)s.nq, np,
	                   (const long long *)d_list_off, items, qidx, obase);
	MVS_HIP(hipGetLastError());
	RangeArgs a;
	memset(&a, 0, sizeof a);
	a.xq = s.xq, a.yb = s.rows;
	a.n = s.nrows, a.nq = (int)s.nq, a.dp = s.dp;
	a.radius = s.radius, a.sel = s.sel, a.idmap = (const long long *)s.idmap_sel, a.rowids = (const long long *)d_rowids;
	a.items = items, a.qidx = qidx, a.obase = obase;
	a.keys = s.keys, a.vals = s.vals, a.cnt = s.cnt, a.cap = s.cap;
	s.metric == METRIC_L2 ? launch_pair<true>(a, (int)npairs, st) : launch_pair<false>(a, (int)npairs, st); // IVFFlatScanner: per-pair arithmetic
}

void RangeResult::clear(int64_t nq) {
	lims.assign((size_t)std::max<int64_t>(nq, 0) + 1, 0);
	distances.clear();
	labels.clear();
}

// One chunk of queries [q0, q0 + nq): scan (twice when the stream was too small), sort, lims, labels, three D2H copies behind `out`.
void range_collect(RangeWork &w, RangeScan s, const std::function<void(const RangeScan &)> &scan, int64_t q0, const int64_t *d_rowids,
                   const int64_t *d_idmap_out, int64_t label_offset, RangeResult &out, hipStream_t st) {
	const int64_t nq = s.nq;
	int64_t cap = w.stream_cap > 0 ? w.stream_cap : std::max<int64_t>((int64_t)1 << 20, nq * 256);
	w.ctl.reserve(64 + (size_t)(nq + 1) * sizeof(long long));
	unsigned long long *d_cnt = (unsigned long long *)w.ctl.p;
	long long *d_lims = (long long *)((char *)w.ctl.p + 64);
	unsigned long long cnt = 0;
	for (int pass = 0; pass < 2; ++pass) {
		w.keys.reserve((size_t)cap * 8);
		w.vals.reserve((size_t)cap * 8);
		MVS_HIP(hipMemsetAsync(d_cnt, 0, 8, st));
		s.keys = (unsigned long long *)w.keys.p, s.vals = (unsigned long long *)w.vals.p, s.cnt = d_cnt, s.cap = cap;
		scan(s);
		MVS_HIP(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, st));
		MVS_HIP(hipStreamSynchronize(st));
		const int64_t before = (int64_t)out.distances.size();
		if (before + (int64_t)cnt > ((int64_t)1 << 30))
			throw_faiss("mvs::range_search", __FILE__, "%lld hits (so far) within radius %g exceed the 2^30 entries one call returns",
			            (long long)(before + (int64_t)cnt), (double)s.radius);
		if ((int64_t)cnt <= cap)
			break;
		if (pass == 1) // (the scan is deterministic: the second one was sized by the first one's count)
			throw_faiss("mvs::range_search", __FILE__, "the hit stream overflowed twice (%lld entries, capacity %lld)", (long long)cnt,
			            (long long)cap);
		cap = (int64_t)cnt; // the exact size, and the same scan once more
		++w.rescans;
	}
	const size_t base = out.distances.size();
	for (int64_t q = 0; q <= nq; ++q)
		out.lims[(size_t)(q0 + q)] = (int64_t)base;
	if (cnt == 0)
		return;
	const int64_t n = (int64_t)cnt;
	w.skeys.reserve((size_t)n * 8);
	w.svals.reserve((size_t)n * 8);
	const int end_bit = 32 + range_qbits(nq);
	size_t temp_bytes = 0;
	MVS_HIP(rocprim::radix_sort_pairs(nullptr, temp_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
	                                  (unsigned long long *)nullptr, (size_t)n, 0, end_bit, st));
	w.temp.reserve(std::max<size_t>(temp_bytes, 16));
	MVS_HIP(rocprim::radix_sort_pairs(w.temp.p, temp_bytes, (unsigned long long *)w.keys.p, (unsigned long long *)w.skeys.p,
	                                  (unsigned long long *)w.vals.p, (unsigned long long *)w.svals.p, (size_t)n, 0, end_bit, st));
	hipLaunchKernelGGL(range_lims_kernel, dim3((unsigned)((nq + 1 + 255) / 256)), dim3(256), 0, st, (const unsigned long long *)w.skeys.p,
	                   (long long)n, (int)nq, d_lims);
	// the unsorted stream is dead: its buffers take the distances and the labels
	float *d_D = (float *)w.vals.p;
	long long *d_I = (long long *)w.keys.p;
	hipLaunchKernelGGL(range_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const unsigned long long *)w.svals.p, (long long)n,
	                   (const long long *)d_rowids, (const long long *)d_idmap_out, (long long)label_offset, d_D, d_I);
	MVS_HIP(hipGetLastError());
	std::vector<long long> lims((size_t)nq + 1);
	out.distances.resize(base + (size_t)n);
	out.labels.resize(base + (size_t)n);
	MVS_HIP(hipMemcpyAsync(lims.data(), d_lims, lims.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
	MVS_HIP(hipMemcpyAsync(out.distances.data() + base, d_D, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
	MVS_HIP(hipMemcpyAsync(out.labels.data() + base, d_I, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
	MVS_HIP(hipStreamSynchronize(st));
	for (int64_t q = 0; q <= nq; ++q)
		out.lims[(size_t)(q0 + q)] = (int64_t)base + lims[(size_t)q];
}

// ------------------------------------------------------------------------------------------------------------------------- Flat
// IndexFlat::range_search.  dis is what search_flat computes for the same batch: a selector or fewer than 20 queries -> the per-pair
// chains; otherwise the BLAS-branch value (MFMA kernel at dp <= 128 unless option range_mfma = 0, else the VALU formula mode).
void FlatIndex::range_search_mapped(int64_t nq, const float *d_x, float radius, const mvs_search_params *params, const int64_t *d_idmap,
                                    RangeResult &out, hipStream_t st) {
	use_device();
	TraceRange tr("mvs:flat_range_search");
	if (metric_is_extra(metric))
		throw_faiss("virtual void faiss::Index::range_search(...) const", "faiss/Index.cpp", "range search not implemented");
	if (!retired.empty())
		reap_retired(false);
	if (flush_adds()) // (rows staged by add() reach the device before anything reads them)
		stream_wait(st, stream);
	out.clear(nq);
	if (nq <= 0 || ntotal == 0)
		return;
	if (ntotal >= ((int64_t)1 << 32)) // (ordinal and payload position are 32-bit fields; FlatIndex::add stops far below)
		throw_faiss("mvs::FlatIndex::range_search", __FILE__, "an index of %lld rows is beyond the 2^32 rows a range search numbers", (long long)ntotal);
	// the scratch buffers are shared with the searches of this index: order this call after the last one
	if (have_last_search)
		stream_wait(st, last_search_stream);
	last_search_stream = st;
	have_last_search = true;
	const bool has_sel = params && params->sel_kind != MVS_SEL_NONE;
	const bool pair = has_sel || nq < 20; // FlatIndex::search_flat's dispatch, on the WHOLE batch
	const bool mfma = !pair && range_use_mfma && range_mfma_supported(geom);
	const bool formula = !pair && metric == METRIC_L2;
	SelectorDev sel = selector.upload(params, sel_domain(d_idmap), st);
	memset(&kinfo, 0, sizeof kinfo);
	const int64_t chunk = 65536; // query index and ordinal fit 32 bits each; the padded queries stay below 32 MB x dp / 128
	int grid = 0;
	for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
		const int64_t nc = std::min(chunk, nq - q0);
		const int64_t nq_pad = (nc + QBLOCK - 1) / QBLOCK * QBLOCK;
		ws_q.reserve((size_t)nq_pad * geom.dp * sizeof(float));
		MVS_HIP(hipMemsetAsync(ws_q.p, 0, (size_t)nq_pad * geom.dp * sizeof(float), st));
		launch_pad_rows(d_x + (size_t)q0 * d, nc, d, (float *)ws_q.p, geom.dp, st);
		RangeScan s;
		memset(&s, 0, sizeof s);
		s.metric = metric, s.nq = nc, s.xq = (const float *)ws_q.p, s.rows = vecs(), s.norms = norms(), s.nrows = ntotal, s.dp = geom.dp;
		s.interleaved = geom.pair_interleaved, s.formula = formula, s.radius = radius, s.sel = sel, s.idmap_sel = d_idmap;
		if (formula) {
			ws_qn.reserve((size_t)nc * sizeof(float));
			launch_query_norms(d_x + (size_t)q0 * d, nc, d, (float *)ws_qn.p, st);
			s.xn = (const float *)ws_qn.p;
		}
		range_collect(range_work, s, [&](const RangeScan &sc) {
			begin_kernel_timing(st);
			launch_range_flat(sc, mfma, &grid, st);
			end_kernel_timing(st);
		}, q0, nullptr, d_idmap, d_idmap ? 0 : label_offset, out, st);
	}
	const int64_t ngroups = mfma ? (nq + QBLOCK - 1) / QBLOCK : (nq + RQ - 1) / RQ;
	set_kinfo(mfma ? "range_mfma_kernel" : "range_pair_kernel", 2.0 * (double)nq * (double)ntotal * d * (pair && metric == METRIC_L2 ? 1.5 : 1.0),
	          (double)ngroups * (double)ntotal * geom.dp * 4.0, grid, 256, mfma ? 2 * (64 * (geom.dp + 1) + 64) * 4 : RTILE * (std::min(geom.dp, 32) + 1) * 4, 0);
}

} // namespace mvs
