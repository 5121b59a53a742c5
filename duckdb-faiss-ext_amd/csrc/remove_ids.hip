// csrc/remove_ids.hip -- the device side of remove_ids (include/mi355_faiss.h "remove_ids") and the host code the index
// kinds share.  A removal is a stable compaction (Flat, PQ, SQ8, the id map of IDMap) or a gather by the host plan's permutation (the IVF
// kinds, csrc/remove_plan.h), always OUT OF PLACE into a fresh allocation: if that allocation fails the index is as before.
//
// Kernels
//   remove_mark_kernel          one thread per row: flag = 1 unless the row's id (label_offset + r, or id_map[r]) is a member of the selector
//   (rocprim exclusive_scan)    flags -> destinations; entry n is the survivor count.  No atomics: the order comes from the scan
//   remove_compact_rows_kernel  rows of `pitch` bytes as uint4: one lane per 16 bytes, consecutive lanes on consecutive words, so a wave
//                               instruction covers 1024 contiguous bytes of one row or of adjacent rows; lanes of removed rows load nothing
//   remove_compact_i64_kernel   the same for the int64 id map
//   remove_compact_flat_kernel  the Flat f32 store and its norms.  In the pair-interleaved layout the place of a float inside its group of
//                               four depends on bit 4 of the ROW NUMBER ([k0,k2,k1,k3] clear, [k1,k3,k0,k2] set): a survivor whose new number
//                               has the other bit 4 gets the two halves of every group swapped on the way
//   remove_gather_rows_kernel   dst row i = src row perm[i], rows as uint4
#include "coded_lists.h"
#include "remove_plan.h"
#include "selector_program.h"

#include <rocprim/device/device_scan.hpp>

#include <chrono>
#include <cstdlib>
#include <cstring>

namespace mvs {

namespace {

constexpr unsigned MAX_BLOCKS = 1u << 20; // (grid-stride loops: a grid never exceeds this)

__device__ __forceinline__ bool remove_sel_member(const SelectorDev &s, long long id) {
	if (s.kind == MVS_SEL_BITMAP) {
		const unsigned long long u = (unsigned long long)id;
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

// flags [n + 1]; entry n = 0 so that the exclusive scan's entry n is the survivor count
__global__ __launch_bounds__(256) void remove_mark_kernel(SelectorDev sel, const long long *__restrict__ idmap, long long off, long long n,
                                                          unsigned *__restrict__ flags) {
	for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += (long long)gridDim.x * blockDim.x) {
		unsigned keep = 0;
		if (r < n)
			keep = remove_sel_member(sel, idmap ? idmap[r] : off + r) ? 0u : 1u;
		flags[r] = keep;
	}
}

__global__ __launch_bounds__(256) void remove_compact_rows_kernel(const uint4 *__restrict__ src, const unsigned *__restrict__ flags,
                                                                  const unsigned *__restrict__ dest, long long n, int words, uint4 *__restrict__ dst) {
	const long long total = n * words;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const long long r = i / words;
		if (!flags[r])
			continue;
		const int w = (int)(i - r * words);
		dst[(long long)dest[r] * words + w] = src[i];
	}
}

__global__ __launch_bounds__(256) void remove_compact_i64_kernel(const long long *__restrict__ src, const unsigned *__restrict__ flags,
                                                                 const unsigned *__restrict__ dest, long long n, long long *__restrict__ dst) {
	for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x)
		if (flags[r])
			dst[dest[r]] = src[r];
}

// cpr: groups of four floats per row (dp / 4)
__global__ __launch_bounds__(256) void remove_compact_flat_kernel(const float4 *__restrict__ src, const float *__restrict__ norms,
                                                                  const unsigned *__restrict__ flags, const unsigned *__restrict__ dest, long long n,
                                                                  int cpr, int interleave, float4 *__restrict__ dst, float *__restrict__ dst_norms) {
	const long long total = n * cpr;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const long long r = i / cpr;
		if (!flags[r])
			continue;
		const int g = (int)(i - r * cpr);
		const long long nr = dest[r];
		float4 v = src[i];
		if (interleave && (((r ^ nr) >> 4) & 1)) // [k0,k2,k1,k3] <-> [k1,k3,k0,k2]: the halves change places
			v = make_float4(v.z, v.w, v.x, v.y);
		dst[nr * cpr + g] = v;
		if (g == 0)
			dst_norms[nr] = norms[r];
	}
}

__global__ __launch_bounds__(256) void remove_gather_rows_kernel(const uint4 *__restrict__ src, const int *__restrict__ perm, long long n, int words,
                                                                 uint4 *__restrict__ dst) {
	const long long total = n * words;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const long long r = i / words;
		const int w = (int)(i - r * words);
		dst[i] = src[(long long)perm[r] * words + w];
	}
}

unsigned grid_for(long long total) {
	return (unsigned)std::max<long long>(1, std::min<long long>((total + 255) / 256, (long long)MAX_BLOCKS));
}

// flags [n + 1] are in place: dest = their exclusive scan; the survivor count comes back
int64_t scan_marks(RemoveMarks &m, hipStream_t st) {
	size_t bytes = 0;
	MVS_HIP(rocprim::exclusive_scan(nullptr, bytes, (unsigned *)nullptr, (unsigned *)nullptr, 0u, (size_t)m.n + 1, rocprim::plus<unsigned>(), st));
	m.temp.reserve(std::max<size_t>(bytes, 16));
	MVS_HIP(rocprim::exclusive_scan(m.temp.p, bytes, (unsigned *)m.flags.p, (unsigned *)m.dest.p, 0u, (size_t)m.n + 1, rocprim::plus<unsigned>(), st));
	unsigned nkeep = 0;
	MVS_HIP(hipMemcpyAsync(&nkeep, (unsigned *)m.dest.p + m.n, sizeof nkeep, hipMemcpyDeviceToHost, st));
	MVS_HIP(hipStreamSynchronize(st));
	m.nkeep = (int64_t)nkeep;
	return m.nkeep;
}

} // namespace

void check_remove_selector(const mvs_search_params *sel) {
	if (sel && sel->sel_kind == MVS_SEL_PROGRAM) { // (include/mi355_faiss.h "selector programs")
		const std::string err = sel_program_validate((const mvs_sel_node *)sel->sel_data, sel->sel_n);
		if (!err.empty())
			throw_faiss("faiss::Index::remove_ids", __FILE__, "selector program: %s", err.c_str());
		return;
	}
	if (!sel || (sel->sel_kind != MVS_SEL_BITMAP && sel->sel_kind != MVS_SEL_BATCH))
		throw_faiss("faiss::Index::remove_ids", __FILE__, "remove_ids needs an IDSelectorBitmap (MVS_SEL_BITMAP) or an IDSelectorBatch (MVS_SEL_BATCH): selector kind %d",
		            sel ? (int)sel->sel_kind : 0);
	if (sel->sel_n < 0 || (sel->sel_n > 0 && !sel->sel_data))
		throw_faiss("faiss::Index::remove_ids", __FILE__, "remove_ids: a selector of %lld entries without data", (long long)sel->sel_n);
}

int64_t remove_mark(RemoveMarks &m, SelectorDev sel, const int64_t *d_idmap, int64_t label_offset, int64_t n, hipStream_t st) {
	m.n = n;
	m.flags.reserve((size_t)(n + 1) * sizeof(unsigned));
	m.dest.reserve((size_t)(n + 1) * sizeof(unsigned));
	hipLaunchKernelGGL(remove_mark_kernel, dim3(grid_for(n + 1)), dim3(256), 0, st, sel, (const long long *)d_idmap, (long long)label_offset, (long long)n,
	                   (unsigned *)m.flags.p);
	MVS_HIP(hipGetLastError());
	return scan_marks(m, st);
}

int64_t remove_marks_from_host(RemoveMarks &m, const uint8_t *keep, int64_t n, hipStream_t st) {
	m.n = n;
	m.flags.reserve((size_t)(n + 1) * sizeof(unsigned));
	m.dest.reserve((size_t)(n + 1) * sizeof(unsigned));
	std::vector<unsigned> f((size_t)n + 1, 0u);
	for (int64_t i = 0; i < n; ++i)
		f[(size_t)i] = keep[i] ? 1u : 0u;
	MVS_HIP(hipMemcpyAsync(m.flags.p, f.data(), f.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
	return scan_marks(m, st); // (synchronises: `f` may go)
}

void launch_remove_compact_rows(const void *d_src, int pitch, const RemoveMarks &m, void *d_dst, hipStream_t st) {
	if (m.n <= 0 || m.nkeep <= 0)
		return;
	const int words = pitch / 16;
	hipLaunchKernelGGL(remove_compact_rows_kernel, dim3(grid_for((long long)m.n * words)), dim3(256), 0, st, (const uint4 *)d_src,
	                   (const unsigned *)m.flags.p, (const unsigned *)m.dest.p, (long long)m.n, words, (uint4 *)d_dst);
	MVS_HIP(hipGetLastError());
}

void launch_remove_compact_i64(const int64_t *d_src, const RemoveMarks &m, int64_t *d_dst, hipStream_t st) {
	if (m.n <= 0 || m.nkeep <= 0)
		return;
	hipLaunchKernelGGL(remove_compact_i64_kernel, dim3(grid_for(m.n)), dim3(256), 0, st, (const long long *)d_src, (const unsigned *)m.flags.p,
	                   (const unsigned *)m.dest.p, (long long)m.n, (long long *)d_dst);
	MVS_HIP(hipGetLastError());
}

void launch_remove_compact_flat(const FlatGeom &g, const float *d_vecs, const float *d_norms, const RemoveMarks &m, float *d_dst, float *d_dst_norms,
                                hipStream_t st) {
	if (m.n <= 0 || m.nkeep <= 0)
		return;
	const int cpr = g.dp / 4;
	hipLaunchKernelGGL(remove_compact_flat_kernel, dim3(grid_for((long long)m.n * cpr)), dim3(256), 0, st, (const float4 *)d_vecs, d_norms,
	                   (const unsigned *)m.flags.p, (const unsigned *)m.dest.p, (long long)m.n, cpr, g.pair_interleaved ? 1 : 0, (float4 *)d_dst,
	                   d_dst_norms);
	MVS_HIP(hipGetLastError());
}

void launch_remove_gather_rows(const void *d_src, const int *d_perm, int64_t n, int pitch, void *d_dst, hipStream_t st) {
	if (n <= 0)
		return;
	const int words = pitch / 16;
	hipLaunchKernelGGL(remove_gather_rows_kernel, dim3(grid_for((long long)n * words)), dim3(256), 0, st, (const uint4 *)d_src, d_perm, (long long)n, words,
	                   (uint4 *)d_dst);
	MVS_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------- code store
void CodeStore::compact(const RemoveMarks &m, hipStream_t stream) {
	DevMem nb((size_t)cap * pitch); // (throws before anything changed)
	MVS_HIP(hipMemsetAsync(nb.p, 0, nb.cap, stream));
	launch_remove_compact_rows(codes(), pitch, m, (unsigned char *)nb.p, stream);
	MVS_HIP(hipStreamSynchronize(stream));
	mem = std::move(nb);
}
void CodeStore::gather(const std::vector<int32_t> &perm, hipStream_t stream) {
	DevMem nb((size_t)cap * pitch);
	DevBuf dperm;
	dperm.reserve(std::max<size_t>(perm.size() * sizeof(int32_t), 16));
	MVS_HIP(hipMemsetAsync(nb.p, 0, nb.cap, stream));
	if (!perm.empty())
		MVS_HIP(hipMemcpyAsync(dperm.p, perm.data(), perm.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
	launch_remove_gather_rows(codes(), (const int *)dperm.p, (int64_t)perm.size(), pitch, (unsigned char *)nb.p, stream);
	MVS_HIP(hipStreamSynchronize(stream));
	mem = std::move(nb);
}

// ---------------------------------------------------------------------------------------------- the IVF kinds' host side
bool ivf_remove_plan_host(const ListDirectory &dir, const mvs_search_params *sel, const int64_t *d_idmap, RemoveMarks *marks, IvfRemovePlan &plan,
                          hipStream_t st) {
	const std::vector<int64_t> &ids_h = dir.ids;
	const int64_t n = dir.rows();
	// (MVS_REMOVE_PROFILE=1: where the host side's time goes, on stderr -- tools/remove_bench.py)
	const bool prof = getenv("MVS_REMOVE_PROFILE") != nullptr;
	auto t_prev = std::chrono::steady_clock::now();
	auto lap = [&](const char *what) {
		if (!prof)
			return;
		const auto t = std::chrono::steady_clock::now();
		fprintf(stderr, "removeprofile\tIVF host %s: %.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count());
		t_prev = t;
	};
	// (a program is evaluated here, on the host, where the plan is made: the stored ids are host data, and no scan follows that a lowered
	// selector would serve)
	const bool is_prog = sel->sel_kind == MVS_SEL_PROGRAM;
	const RemoveSelector plain(is_prog ? 0 : sel->sel_kind, sel->sel_data, is_prog ? 0 : sel->sel_n);
	SelProgram prog;
	if (is_prog)
		sel_program_pack((const mvs_sel_node *)sel->sel_data, sel->sel_n, prog);
	struct {
		const RemoveSelector &plain;
		const SelProgram *prog;
		bool member(int64_t id) const {
			return prog ? sel_program_member(*prog, id) : plain.member(id);
		}
	} rs {plain, is_prog ? &prog : nullptr};
	lap("selector sort");
	std::vector<uint8_t> keep((size_t)n);
	std::vector<int64_t> renum;
	bool any = false;
	if (d_idmap) {
		// IDMap over an IVF kind: the stored id s names id_map[s].  The survivors are renumbered so that it still does -- which needs the
		// stored ids to be exactly 0 .. ntotal-1
		if (!remove_ids_are_permutation(ids_h))
			throw_faiss("faiss::IndexIDMap::remove_ids", __FILE__, "remove_ids under IDMap needs the sub-index's stored ids to be exactly 0 .. ntotal-1, "
			            "each once: this index (read from a foreign file?) stores others");
		std::vector<int64_t> idm((size_t)n);
		MVS_HIP(hipMemcpyAsync(idm.data(), d_idmap, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
		MVS_HIP(hipStreamSynchronize(st));
		std::vector<uint8_t> keep_by_id((size_t)n);
		for (int64_t s = 0; s < n; ++s) {
			keep_by_id[(size_t)s] = rs.member(idm[(size_t)s]) ? 0 : 1;
			any = any || !keep_by_id[(size_t)s];
		}
		if (!any)
			return false;
		for (int64_t i = 0; i < n; ++i)
			keep[(size_t)i] = keep_by_id[(size_t)ids_h[(size_t)i]];
		renum = remove_renumber(keep_by_id);
		if (marks)
			remove_marks_from_host(*marks, keep_by_id.data(), n, st);
	} else {
		for (int64_t i = 0; i < n; ++i) {
			keep[(size_t)i] = rs.member(ids_h[(size_t)i]) ? 0 : 1;
			any = any || !keep[(size_t)i];
		}
		if (!any)
			return false;
	}
	lap("membership");
	ivf_remove_plan(dir.nlist, dir.assign, ids_h, keep, d_idmap ? &renum : nullptr, plan);
	lap("swap loops + new arrival order");
	return true;
}

} // namespace mvs
