// csrc/reconstruct.hip -- faiss::Index::reconstruct, reconstruct_n, reconstruct_batch and search_and_reconstruct for every index kind
// (include/mi355_faiss.h "reconstruct").  A kind says where its rows live and how a key names one (IndexBase::recon_source,
// a ReconSource); everything else is here once: the lookup table, the resolve kernel, one family of gather / decode kernels, and the
// entry points, which stage keys and rows through the index's pinned ring in chunks.
//
// Kernels
//   recon_iota_kernel       positions 0 .. n-1, the values of the table's sort
//   (rocprim radix_sort_pairs)  (key, position) by key; the sort is stable, so equal keys stay in ascending position
//   recon_resolve_kernel    one lane per key: every stage of the source in turn -- a table stage takes the LAST entry of the key's run
//                           (the row added last), a stage without a table checks key - off against [0, n).  A lane whose key names no
//                           row lowers the miss word to its batch index with an atomic; the host reads that one word after the gather
//   recon_gather_kernel<MODE, LDS>  positions -> [n][d] dense f32.  2^j lanes (4 floats each, up to a whole wave) own an output row;
//                           a lane loads 16 bytes of an f32 row (4 code bytes of a coded one) and stores 16 bytes where d % 4 == 0 and the
//                           output is aligned, single floats otherwise.  RECON_F32 undoes the pair-interleaved layout by the row's
//                           bit 4; RECON_SQ8 decodes a + (float)c s; RECON_PQ copies codebook entries, from LDS (LDS = true: the
//                           workgroup, of 1024 lanes, loads the 1024 d bytes of codebooks once and walks rows with a grid stride) or through L2.  A
//                           coded IVF kind adds its list's centroid to the decoded residual, one f32 addition.  No operation here may
//                           be contracted: the arithmetic is csrc/sq8_kernels.h's sq_add / sq_mul.
//                           position -1: the row is left untouched; -2: every byte 0xFF (a label of -1)
#include "coded_lists.h"
#include "sq8_kernels.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <cstdlib>
#include <cstring>

namespace mvs {

namespace {

constexpr unsigned RECON_MAX_BLOCKS = 1u << 16;        // (grid-stride loops: a grid never exceeds this)
constexpr size_t RECON_PQ_LDS_MAX = (size_t)128 << 10; // codebooks of at most this many bytes (d <= 128) may go to LDS
constexpr int64_t RECON_STAGE_BYTES = (int64_t)PinnedRing::SLOT_BYTES; // rows staged per chunk of a host call
constexpr int64_t RECON_DEVICE_KEYS = (int64_t)1 << 22; // keys resolved per launch of a device-resident call
constexpr unsigned RECON_NO_MISS = 0xFFFFFFFFu;

struct ResolveArgs {
	ReconStage stage[2];
	int nstage, policy;
	const long long *keys; // null: i0 + i
	long long i0, n;
	long long *pos;
	unsigned *miss;
};

__global__ __launch_bounds__(256) void recon_iota_kernel(unsigned *__restrict__ v, long long n) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
		v[i] = (unsigned)i;
}

__global__ __launch_bounds__(256) void recon_resolve_kernel(ResolveArgs a) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (long long)gridDim.x * blockDim.x) {
		long long p = a.keys ? a.keys[i] : a.i0 + i;
		if ((a.policy == RECON_PAD || a.policy == RECON_PAD_UNCHECKED) && p == -1) {
			a.pos[i] = -2;
			continue;
		}
		bool found = true;
		for (int s = 0; s < a.nstage && found; ++s) {
			const ReconStage &t = a.stage[s];
			if (!t.keys) {
				p -= t.off;
				found = p >= 0 && p < t.n;
				continue;
			}
			long long lo = 0, hi = t.n; // upper bound: the first entry beyond the key
			while (lo < hi) {
				const long long mid = (lo + hi) >> 1;
				if (t.keys[mid] <= p)
					lo = mid + 1;
				else
					hi = mid;
			}
			found = lo > 0 && t.keys[lo - 1] == p;
			if (found)
				p = (long long)t.pos[lo - 1];
		}
		if (!found) {
			p = a.policy == RECON_PAD_UNCHECKED ? -2 : -1;
			if (a.policy == RECON_STRICT || a.policy == RECON_PAD)
				atomicMin(a.miss, (unsigned)i);
		}
		a.pos[i] = p;
	}
}

struct GatherArgs {
	const unsigned char *rows;
	long long pitch, n;
	const long long *pos;
	float *out;
	const float *sq_a, *sq_s, *cb, *cent;
	const int *assign;
	int d, ngroups, lpr, interleaved, vec, dvec, cbvec, M, dsub, cb_float4s;
};

// p[k .. k + 3] of a table of d floats per row: one 16-byte load where d % 4 == 0 (the row starts are then 16-byte aligned), else guarded singles
__device__ __forceinline__ void recon_load4(const float *__restrict__ p, int k, int d, int dvec, float o[4]) {
	if (dvec) {
		const float4 w = *reinterpret_cast<const float4 *>(p + k);
		o[0] = w.x, o[1] = w.y, o[2] = w.z, o[3] = w.w;
	} else {
#pragma unroll
		for (int e = 0; e < 4; ++e)
			o[e] = k + e < d ? p[k + e] : 0.f;
	}
}

template <int MODE, bool LDS>
__global__ __launch_bounds__(1024) void recon_gather_kernel(GatherArgs a) {
	extern __shared__ __attribute__((aligned(16))) float4 recon_lds[]; // (the only LDS of the kernel: its base is 16-byte aligned)
	if (LDS) {
		const float4 *src = reinterpret_cast<const float4 *>(a.cb);
		for (int i = threadIdx.x; i < a.cb_float4s; i += blockDim.x)
			recon_lds[i] = src[i];
		__syncthreads();
	}
	const float *cb = LDS ? reinterpret_cast<const float *>(recon_lds) : a.cb;
	const int rpb = blockDim.x / a.lpr, sub = threadIdx.x / a.lpr, lane = threadIdx.x - sub * a.lpr;
	for (long long r = (long long)blockIdx.x * rpb + sub; r < a.n; r += (long long)gridDim.x * rpb) {
		const long long p = a.pos[r];
		if (p == -1)
			continue;
		float *o = a.out + r * a.d;
		const unsigned char *row = a.rows + (p < 0 ? 0 : p) * a.pitch;
		const float *cent = nullptr;
		if (MODE != RECON_F32 && a.cent && p >= 0) {
			const int l = a.assign[p];
			if (l >= 0)
				cent = a.cent + (long long)l * a.d;
		}
		for (int g = lane; g < a.ngroups; g += a.lpr) {
			const int k = g * 4;
			float v[4];
			if (p < 0) {
				v[0] = v[1] = v[2] = v[3] = __uint_as_float(0xFFFFFFFFu);
			} else if (MODE == RECON_F32) {
				const float4 w = reinterpret_cast<const float4 *>(row)[g];
				if (!a.interleaved)
					v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
				else if ((p >> 4) & 1) // stored [k1,k3,k0,k2]
					v[0] = w.z, v[1] = w.x, v[2] = w.w, v[3] = w.y;
				else // stored [k0,k2,k1,k3]
					v[0] = w.x, v[1] = w.z, v[2] = w.y, v[3] = w.w;
			} else if (MODE == RECON_SQ8) {
				const unsigned c4 = reinterpret_cast<const unsigned *>(row)[g];
				float qa[4], qs[4];
				recon_load4(a.sq_a, k, a.d, a.dvec, qa);
				recon_load4(a.sq_s, k, a.d, a.dvec, qs);
#pragma unroll
				for (int e = 0; e < 4; ++e)
					v[e] = sq_add(qa[e], sq_mul((float)((c4 >> (8 * e)) & 0xFFu), qs[e]));
			} else if (a.cbvec) { // four floats of one codebook entry
				const int m = k / a.dsub, j = k - m * a.dsub;
				const float4 w = *reinterpret_cast<const float4 *>(cb + ((long long)m * 256 + row[m]) * a.dsub + j);
				v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
			} else {
#pragma unroll
				for (int e = 0; e < 4; ++e) {
					v[e] = 0.f;
					if (k + e < a.d) {
						const int m = (k + e) / a.dsub, j = k + e - m * a.dsub;
						v[e] = cb[((long long)m * 256 + row[m]) * a.dsub + j];
					}
				}
			}
			if (MODE != RECON_F32 && cent) {
				float c[4];
				recon_load4(cent, k, a.d, a.dvec, c);
#pragma unroll
				for (int e = 0; e < 4; ++e)
					v[e] = sq_add(v[e], c[e]);
			}
			if (a.vec) {
				reinterpret_cast<float4 *>(o)[g] = make_float4(v[0], v[1], v[2], v[3]);
			} else {
#pragma unroll
				for (int e = 0; e < 4; ++e)
					if (k + e < a.d)
						o[k + e] = v[e];
			}
		}
	}
}

unsigned grid_for(long long items, int per_block) {
	return (unsigned)std::max<long long>(1, std::min<long long>((items + per_block - 1) / per_block, (long long)RECON_MAX_BLOCKS));
}

// -> the PQ branch taken (1: codebooks in LDS, 0: through L2), -1 for the other modes
int launch_gather(const ReconSource &s, int d, int64_t n, const long long *d_pos, float *d_out, hipStream_t st) {
	GatherArgs a;
	memset(&a, 0, sizeof a);
	a.rows = (const unsigned char *)s.rows;
	a.pitch = s.pitch, a.n = n, a.pos = d_pos, a.out = d_out;
	a.sq_a = s.sq_a, a.sq_s = s.sq_s, a.cb = s.cb, a.cent = s.cent, a.assign = s.assign;
	a.d = d, a.ngroups = (d + 3) / 4;
	a.lpr = 1;
	while (a.lpr < a.ngroups && a.lpr < 64)
		a.lpr <<= 1;
	a.interleaved = s.interleaved;
	a.dvec = d % 4 == 0;
	a.vec = a.dvec && ((uintptr_t)d_out & 15) == 0;
	a.M = s.M, a.dsub = s.dsub;
	a.cbvec = s.mode == RECON_PQ && s.dsub % 4 == 0;
	const int rpb = 256 / a.lpr;
	unsigned grid = grid_for(n, rpb);
	int branch = -1;
	if (s.mode == RECON_F32) {
		hipLaunchKernelGGL((recon_gather_kernel<RECON_F32, false>), dim3(grid), dim3(256), 0, st, a);
	} else if (s.mode == RECON_SQ8) {
		hipLaunchKernelGGL((recon_gather_kernel<RECON_SQ8, false>), dim3(grid), dim3(256), 0, st, a);
	} else {
		// the codebooks go to LDS when they fit and the rows written are at least as many bytes as the codebooks every workgroup loads
		const size_t cb_bytes = (size_t)s.M * 256 * s.dsub * sizeof(float);
		bool lds = s.cb && cb_bytes <= RECON_PQ_LDS_MAX && (size_t)n * d * sizeof(float) >= cb_bytes;
		if (const char *e = getenv("MVS_RECON_PQ_LDS")) // (measurement: 0 forces the L2 branch, 1 the LDS branch where the codebooks fit -- tools/reconstruct_bench.py)
			lds = s.cb && cb_bytes <= RECON_PQ_LDS_MAX && atoi(e) != 0;
		branch = lds ? 1 : 0;
		if (lds) {
			// one resident workgroup per compute unit, each loads the codebooks once; 1024 lanes, so that 16 wavefronts' row fetches are in
			// flight per compute unit (with 256 lanes the walk waited for memory: 1.16 ms for 1 M rows of IVF4096,PQ16, profiles/reconstruct.txt)
			a.cb_float4s = (int)(cb_bytes / 16);
			grid = std::min<unsigned>(grid_for(n, 1024 / a.lpr), 256u);
			ensure_dynamic_lds((const void *)recon_gather_kernel<RECON_PQ, true>, cb_bytes);
			hipLaunchKernelGGL((recon_gather_kernel<RECON_PQ, true>), dim3(grid), dim3(1024), cb_bytes, st, a);
		} else {
			hipLaunchKernelGGL((recon_gather_kernel<RECON_PQ, false>), dim3(grid), dim3(256), 0, st, a);
		}
	}
	MVS_HIP(hipGetLastError());
	return branch;
}

void check_keys(int64_t n) { // the 2^31 guard: a batch index travels in 32 bits
	if (n > (int64_t)0x7fffffff - 1024)
		throw_faiss("mvs::IndexBase::reconstruct_batch", __FILE__, "a reconstruction call takes at most 2^31 keys");
}

} // namespace

// ---------------------------------------------------------------------------------------------- the lookup table
void recon_table_build(ReconTable &t, const int64_t *h_ids, const int64_t *d_ids, const int32_t *h_assign, int64_t n, hipStream_t st) {
	t.drop();
	if (n > 0) {
		DevBuf kin, vin, temp;
		t.keys.reserve((size_t)n * sizeof(int64_t));
		t.pos.reserve((size_t)n * sizeof(unsigned));
		vin.reserve((size_t)n * sizeof(unsigned));
		if (h_ids) {
			kin.reserve((size_t)n * sizeof(int64_t));
			MVS_HIP(hipMemcpyAsync(kin.p, h_ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
			d_ids = (const int64_t *)kin.p;
		}
		hipLaunchKernelGGL(recon_iota_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, (unsigned *)vin.p, (long long)n);
		MVS_HIP(hipGetLastError());
		size_t bytes = 0;
		MVS_HIP(rocprim::radix_sort_pairs(nullptr, bytes, (const long long *)d_ids, (long long *)t.keys.p, (const unsigned *)vin.p, (unsigned *)t.pos.p,
		                                  (size_t)n, 0, 64, st));
		temp.reserve(std::max<size_t>(bytes, 16));
		MVS_HIP(rocprim::radix_sort_pairs(temp.p, bytes, (const long long *)d_ids, (long long *)t.keys.p, (const unsigned *)vin.p, (unsigned *)t.pos.p,
		                                  (size_t)n, 0, 64, st));
		if (h_assign) {
			t.assign.reserve((size_t)n * sizeof(int32_t));
			MVS_HIP(hipMemcpyAsync(t.assign.p, h_assign, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
		}
		MVS_HIP(hipStreamSynchronize(st)); // (the sort's inputs and scratch go; the host vectors may change)
	}
	t.n = n;
}

// ---------------------------------------------------------------------------------------------- base
void IndexBase::recon_source(ReconSource &, hipStream_t) {
	throw_faiss("virtual void faiss::Index::reconstruct(faiss::idx_t, float*) const", "faiss/Index.cpp", "reconstruct not implemented for this type of index");
}

void IndexBase::recon_throw_missing(const ReconSource &src, int64_t key) const {
	if (src.nstage > 0 && !src.stage[0].keys) // a kind without ids: FAISS's range check (IndexFlatCodes::reconstruct_n)
		throw_faiss("virtual void faiss::IndexFlatCodes::reconstruct_n(faiss::idx_t, faiss::idx_t, float*) const", "faiss/IndexFlatCodes.cpp",
		            "Error: 'ni == 0 || (i0 >= 0 && i0 + ni <= ntotal)' failed: key %lld outside [%lld, %lld)", (long long)key,
		            (long long)src.stage[0].off, (long long)(src.stage[0].off + src.stage[0].n));
	throw_faiss("virtual void faiss::Index::reconstruct(faiss::idx_t, float*) const", "faiss/DirectMap.cpp", "key not found: %lld", (long long)key);
}

void IndexBase::recon_workspaces(int64_t nkeys, size_t out_bytes) {
	ws_rkeys.reserve(std::max<size_t>((size_t)nkeys * sizeof(int64_t), 16));
	ws_rpos.reserve(std::max<size_t>((size_t)nkeys * sizeof(int64_t), 16));
	ws_rmiss.reserve(16);
	if (out_bytes)
		ws_rout.reserve(out_bytes);
}

void IndexBase::recon_run(const ReconSource &src, int64_t n, const int64_t *d_keys, int64_t i0, float *d_out, int policy, unsigned *d_miss,
                          hipStream_t st) {
	if (n <= 0)
		return;
	ResolveArgs r;
	memset(&r, 0, sizeof r);
	for (int s = 0; s < src.nstage; ++s)
		r.stage[s] = src.stage[s];
	r.nstage = src.nstage, r.policy = policy;
	r.keys = (const long long *)d_keys, r.i0 = i0, r.n = n;
	r.pos = (long long *)ws_rpos.p;
	r.miss = d_miss;
	hipLaunchKernelGGL(recon_resolve_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, r);
	MVS_HIP(hipGetLastError());
	const int branch = launch_gather(src, d, n, (const long long *)ws_rpos.p, d_out, st);
	if (branch >= 0)
		recon_last_pq_lds = branch;
}

// ---------------------------------------------------------------------------------------------- host entry points
// keys (null: i0 .. i0 + n - 1) -> out, in chunks of one pinned slot of rows.  RECON_SKIP sends the caller's rows down first, so that the
// rows of absent keys come back as they were
void IndexBase::recon_host(const ReconSource &src, int64_t n, const int64_t *keys, int64_t i0, float *out, int policy) {
	if (n <= 0)
		return;
	check_keys(n);
	const size_t row_bytes = (size_t)d * sizeof(float);
	const int64_t chunk = std::max<int64_t>(1, RECON_STAGE_BYTES / (int64_t)row_bytes);
	recon_workspaces(std::min(chunk, n), (size_t)std::min(chunk, n) * row_bytes);
	for (int64_t c0 = 0; c0 < n; c0 += chunk) {
		const int64_t nc = std::min(chunk, n - c0);
		const size_t obytes = (size_t)nc * row_bytes, kbytes = (size_t)nc * sizeof(int64_t);
		MVS_HIP(hipMemsetAsync(ws_rmiss.p, 0xFF, sizeof(unsigned), stream));
		if (keys) {
			const int ks = pinned.acquire(kbytes);
			memcpy(pinned.buf[ks], keys + c0, kbytes);
			MVS_HIP(hipMemcpyAsync(ws_rkeys.p, pinned.buf[ks], kbytes, hipMemcpyHostToDevice, stream));
			pinned.release(ks, stream);
		}
		const int slot = pinned.acquire(obytes + 16);
		char *hb = (char *)pinned.buf[slot];
		if (policy == RECON_SKIP) {
			memcpy(hb, out + c0 * d, obytes);
			MVS_HIP(hipMemcpyAsync(ws_rout.p, hb, obytes, hipMemcpyHostToDevice, stream));
		}
		recon_run(src, nc, keys ? (const int64_t *)ws_rkeys.p : nullptr, i0 + c0, (float *)ws_rout.p, policy, (unsigned *)ws_rmiss.p, stream);
		MVS_HIP(hipMemcpyAsync(hb, ws_rout.p, obytes, hipMemcpyDeviceToHost, stream));
		MVS_HIP(hipMemcpyAsync(hb + obytes, ws_rmiss.p, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
		MVS_HIP(hipStreamSynchronize(stream));
		unsigned miss;
		memcpy(&miss, hb + obytes, sizeof miss);
		if (miss != RECON_NO_MISS) {
			pinned.release(slot, stream);
			recon_throw_missing(src, keys ? keys[c0 + miss] : i0 + c0 + miss);
		}
		memcpy(out + c0 * d, hb, obytes);
		pinned.release(slot, stream);
	}
}

// kinds without ids: positions i0 .. i0 + ni - 1; under IDMap: the external keys of the range, each of which must exist; a bare IVF kind,
// as IndexIVF::reconstruct_n: the rows whose stored id lies in the range, at id - i0, the others left untouched
void IndexBase::reconstruct_n(int64_t i0, int64_t ni, float *out) {
	use_device();
	ReconSource src;
	recon_source(src, stream);
	if (ni <= 0)
		return;
	const bool bare_ivf = src.nstage == 1 && src.stage[0].keys;
	if (!src.stage[0].keys && (i0 < src.stage[0].off || i0 + ni > src.stage[0].off + src.stage[0].n))
		recon_throw_missing(src, i0 < src.stage[0].off ? i0 : i0 + ni - 1);
	recon_host(src, ni, nullptr, i0, out, bare_ivf ? RECON_SKIP : RECON_STRICT);
}

void IndexBase::reconstruct_batch(int64_t n, const int64_t *keys, float *out, int policy) {
	use_device();
	ReconSource src;
	recon_source(src, stream); // (first: a kind that does not serve the call refuses whatever n is)
	recon_host(src, n, keys, 0, out, policy);
}

// ---------------------------------------------------------------------------------------------- device-resident entry points
void IndexBase::reconstruct_batch_device(int64_t n, const int64_t *d_keys, float *d_out, hipStream_t st) {
	use_device();
	ReconSource src;
	recon_source(src, st);
	if (n <= 0)
		return;
	check_keys(n);
	const int64_t chunk = std::min(n, RECON_DEVICE_KEYS);
	recon_workspaces(chunk, 0);
	stream_wait(st, stream); // (the workspaces' last use was on the index's stream)
	MVS_HIP(hipMemsetAsync(ws_rmiss.p, 0xFF, 2 * sizeof(unsigned), st));
	// the miss word is a batch index of its chunk: each chunk lowers a word of its own turn, checked before the next chunk reuses the positions
	for (int64_t c0 = 0; c0 < n; c0 += chunk) {
		const int64_t nc = std::min(chunk, n - c0);
		recon_run(src, nc, d_keys + c0, 0, d_out + c0 * d, RECON_STRICT, (unsigned *)ws_rmiss.p, st);
		const int slot = pinned.acquire(16);
		MVS_HIP(hipMemcpyAsync(pinned.buf[slot], ws_rmiss.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
		MVS_HIP(hipStreamSynchronize(st));
		unsigned miss;
		memcpy(&miss, pinned.buf[slot], sizeof miss);
		pinned.release(slot, st);
		if (miss != RECON_NO_MISS) {
			int64_t key = 0;
			MVS_HIP(hipMemcpy(&key, d_keys + c0 + miss, sizeof key, hipMemcpyDeviceToHost));
			recon_throw_missing(src, key);
		}
	}
	for (int i = 0; i < src.nowners; ++i)
		stream_wait(src.owners[i], st);
	stream_wait(stream, st);
}

// ---------------------------------------------------------------------------------------------- search_and_reconstruct
// The search is the index's own, whole (its arithmetic may depend on the batch); the rows are those its labels name, so with duplicate ids
// the row shown is the last added one.  A label of -1 gives a row of 0xFF bytes
void IndexBase::search_and_reconstruct(int64_t nq, const float *x, int64_t k, float *D, int64_t *I, float *recons, const mvs_search_params *params) {
	use_device();
	{
		ReconSource src;
		recon_source(src, stream);
	}
	search(nq, x, k, D, I, params);
	if (nq > 0)
		reconstruct_batch(nq * k, I, recons, RECON_PAD);
}

void IndexBase::search_and_reconstruct_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, float *d_recons,
                                              const mvs_search_params *params, hipStream_t st) {
	use_device();
	{
		ReconSource probe;
		recon_source(probe, st);
	}
	if (k <= 0)
		throw_faiss("virtual void faiss::Index::search(...) const", "faiss/Index.cpp", "Error: 'k > 0' failed");
	if (nq <= 0)
		return;
	check_keys(nq * k);
	search_device(nq, d_x, k, d_D, d_I, params, st);
	use_device();
	ReconSource src; // (asked again: a source holds good only until the index runs something else)
	recon_source(src, st);
	const int64_t n = nq * k, chunk = std::min(n, RECON_DEVICE_KEYS);
	recon_workspaces(chunk, 0);
	stream_wait(st, stream);
	// the labels are the index's own: nothing is read back (a label that named no row would give a row of 0xFF bytes)
	for (int64_t c0 = 0; c0 < n; c0 += chunk)
		recon_run(src, std::min(chunk, n - c0), d_I + c0, 0, d_recons + c0 * d, RECON_PAD_UNCHECKED, (unsigned *)ws_rmiss.p, st);
	for (int i = 0; i < src.nowners; ++i)
		stream_wait(src.owners[i], st);
	stream_wait(stream, st);
}

// ---------------------------------------------------------------------------------------------- the kinds of csrc/index.hip and csrc/coded_lists.hip
void FlatIndex::recon_source(ReconSource &src, hipStream_t st) {
	use_device();
	flush_adds(); // staged rows reach the device (on the index's stream)
	reap_retired(false);
	stream_wait(st, stream);
	src.mode = RECON_F32;
	src.rows = vecs();
	src.pitch = (long long)geom.dp * (long long)sizeof(float);
	src.nrows = ntotal;
	src.interleaved = geom.pair_interleaved ? 1 : 0;
	src.push_stage({nullptr, nullptr, (long long)ntotal, (long long)label_offset});
	src.own(stream);
}

// IndexIDMap2::reconstruct: the row whose external id is the key, the last added one of several (rev_map overwrites).  "IDMap," serves it
// as "IDMap2," does.  The wrapped kind's own stages follow: none but the range check (its rows are the map's), or an IVF kind's table
void IDMapIndex::recon_source(ReconSource &src, hipStream_t st) {
	use_device();
	flush_ids();
	if (!recon_tab.valid() || recon_tab.n != ntotal)
		recon_table_build(recon_tab, nullptr, ids.get(), nullptr, ntotal, stream);
	stream_wait(st, stream);
	src.push_stage({(const long long *)recon_tab.keys.p, (const unsigned *)recon_tab.pos.p, (long long)recon_tab.n, 0});
	src.own(stream);
	sub->recon_source(src, st);
	use_device();
}

void CodedListsIndex::recon_source(ReconSource &src, hipStream_t st) {
	use_device();
	if (ntotal > 0 && !have_par)
		throw_faiss((std::string(names.cls) + "::reconstruct").c_str(), names.file, "the index holds rows but no parameters to decode them with");
	if (kind == MVS_KIND_IVFPQ) {
		src.mode = RECON_PQ;
		src.cb = d_par();
		src.M = code_size, src.dsub = d / code_size;
	} else {
		src.mode = RECON_SQ8;
		src.sq_a = d_par() ? d_par() + 2 * (size_t)d : nullptr;
		src.sq_s = d_par() ? d_par() + 3 * (size_t)d : nullptr;
	}
	src.rows = store.codes();
	src.pitch = store.pitch;
	src.nrows = ntotal;
	if (coarse) {
		if (!recon_tab.valid() || recon_tab.n != ntotal)
			recon_table_build(recon_tab, dir.ids.data(), nullptr, dir.assign.data(), ntotal, stream);
		src.cent = centroids_dev();
		src.assign = (const int *)recon_tab.assign.p;
		src.push_stage({(const long long *)recon_tab.keys.p, (const unsigned *)recon_tab.pos.p, (long long)recon_tab.n, 0});
	} else {
		src.push_stage({nullptr, nullptr, (long long)ntotal, (long long)label_offset});
	}
	stream_wait(st, stream);
	src.own(stream);
}

} // namespace mvs
