// csrc/coded_lists.hip -- CodedListsIndex (csrc/coded_lists.h): the host driver and the small kernels the kinds with coded inverted
// lists share.  DESIGN.md 3.8 describes the scheme.
//
// Kernels
//   coded_gather_codes_kernel   the list-sorted code view out of the arrival-order store
//   coded_prefix_kernel         per query the exclusive prefix of its probed lists' sizes in rank order: the base of its ORDINALS
//   coded_count / offsets / scatter_kernel   the (query, rank) pairs of one unit grouped by list: a counting sort on the device
//   (the kind's scan kernel)    a workgroup takes (<= Q pairs of one list, <= R positions of it); a value strictly below its query's bound
//                               goes to the query's bucket as (order key, ordinal)
//   pq_select_kernel            (csrc/pq_kernels.h) list + bucket sorted, the k best stay, the k-th key becomes the bound
//   coded_emit_kernel           ordinal -> (rank, position) -> stored id (IDMap: id_map[id]), -1 / FLT_MAX padded
//
// Selection.  csrc/pq.hip's range scheme over PROBE RANKS: [0, 1), [1, 3), [3, 9), ...  An entry's ordinal = rows of the lower ranks' lists +
// its position, so later units only bring larger ordinals than every list member: an entry tied at the bound never reaches the
// stream and the pure order (distance, probe rank, position) comes out by construction.  A unit is (rank span, position window); a bucket
// overflow drops the unit, which is scanned again as two halves of the span, or -- one rank -- as two halves of the window.  One rank and
// <= R positions cannot overflow a bucket of R entries: the result never depends on R or on the bucket size.  A kind may have a unit of ONE
// rank walked in windows [0, R), [R, 3R), [3R, 9R), ... from the start: the first cannot overflow and leaves a bound.
//
// Nothing here does float arithmetic on the rows: the kinds' contraction modes (csrc/sq.hip compiles with contraction off) stay theirs.
#include "coded_lists.h"
#include "pq_kernels.h"
#include "remove_plan.h"

#include <algorithm>
#include <cstring>
#include <functional>

namespace mvs {

namespace {

constexpr int ROWS_PER_WG = PQ_ROWS_PER_WG; // positions of a list one scan workgroup walks = bucket entries (pq_select_kernel's pitch)

// out[i] = codes[perm[i]], rows of `pitch` bytes moved as 16-byte words
__global__ __launch_bounds__(256) void coded_gather_codes_kernel(const uint4 *__restrict__ codes, const int *__restrict__ perm, long long n, int words,
                                                                 uint4 *__restrict__ out) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n * words)
		return;
	const long long r = i / words;
	const int w = (int)(i - r * words);
	out[i] = codes[(long long)perm[r] * words + w];
}

// ---------------------------------------------------------------------------------------------- ordinals
// pref [nq][np + 1]: rows of the lists probed at ranks below r (a -1 probe has none)
__global__ __launch_bounds__(256) void coded_prefix_kernel(const long long *__restrict__ cI, long long nq, int np, const long long *__restrict__ list_off,
                                                           long long nlist, unsigned *__restrict__ pref) {
	const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= nq)
		return;
	unsigned acc = 0;
	for (int r = 0; r < np; ++r) {
		pref[q * (np + 1) + r] = acc;
		const long long l = cI[q * np + r];
		if (l >= 0 && l < nlist)
			acc += (unsigned)(list_off[l + 1] - list_off[l]);
	}
	pref[q * (np + 1) + np] = acc;
}

// ---------------------------------------------------------------------------------------------- grouping
// the pairs (query of the chunk, rank in [ra, rb)) whose list has rows at or beyond position p0, counted per list
__global__ __launch_bounds__(256) void coded_count_kernel(const long long *__restrict__ cI, long long nqc, int np, int ra, int rb,
                                                          const long long *__restrict__ list_off, long long nlist, long long p0, int *__restrict__ cnt) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	const int span = rb - ra;
	if (i >= nqc * span)
		return;
	const long long q = i / span;
	const int r = ra + (int)(i - q * span);
	const long long l = cI[q * np + r];
	if (l >= 0 && l < nlist && list_off[l + 1] - list_off[l] > p0)
		atomicAdd(&cnt[l], 1);
}
// poff [nlist + 1]: first pair of every list; goff [nlist + 1]: first pair GROUP (<= Q pairs) of every list.  One workgroup.
__global__ __launch_bounds__(1024) void coded_offsets_kernel(const int *__restrict__ cnt, int nlist, int Q, int *__restrict__ poff, int *__restrict__ goff) {
	__shared__ int sp[1024], sg[1024];
	const int tid = threadIdx.x;
	const int per = (nlist + 1023) / 1024;
	const int l0 = tid * per, l1 = l0 + per < nlist ? l0 + per : nlist;
	int ap = 0, ag = 0;
	for (int l = l0; l < l1; ++l) {
		ap += cnt[l];
		ag += (cnt[l] + Q - 1) / Q;
	}
	sp[tid] = ap, sg[tid] = ag;
	__syncthreads();
	for (int s = 1; s < 1024; s <<= 1) { // inclusive scan of the 1024 partial sums
		const int vp = tid >= s ? sp[tid - s] : 0, vg = tid >= s ? sg[tid - s] : 0;
		__syncthreads();
		sp[tid] += vp, sg[tid] += vg;
		__syncthreads();
	}
	int bp = sp[tid] - ap, bg = sg[tid] - ag;
	for (int l = l0; l < l1; ++l) {
		poff[l] = bp, goff[l] = bg;
		bp += cnt[l];
		bg += (cnt[l] + Q - 1) / Q;
	}
	if (tid == 1023)
		poff[nlist] = sp[1023], goff[nlist] = sg[1023];
}
__global__ __launch_bounds__(256) void coded_scatter_kernel(const long long *__restrict__ cI, long long nqc, int np, int ra, int rb,
                                                            const long long *__restrict__ list_off, long long nlist, long long p0,
                                                            const int *__restrict__ poff, int *__restrict__ cur, int2 *__restrict__ pairs) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	const int span = rb - ra;
	if (i >= nqc * span)
		return;
	const long long q = i / span;
	const int r = ra + (int)(i - q * span);
	const long long l = cI[q * np + r];
	if (l >= 0 && l < nlist && list_off[l + 1] - list_off[l] > p0)
		pairs[poff[l] + atomicAdd(&cur[l], 1)] = make_int2((int)q, r);
}

// ---------------------------------------------------------------------------------------------- emit
__global__ __launch_bounds__(256) void coded_emit_kernel(const unsigned long long *__restrict__ list, const int *__restrict__ len, int k, long long nqc,
                                                         int descending, const long long *__restrict__ cI, int np, const unsigned *__restrict__ pref,
                                                         const long long *__restrict__ list_off, const long long *__restrict__ lids, long long id0,
                                                         const long long *__restrict__ idmap, float *__restrict__ D, long long *__restrict__ I) {
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nqc * k)
		return;
	const long long q = i / k;
	const int s = (int)(i - q * k);
	if (s < len[q]) {
		const unsigned long long e = list[i];
		const unsigned ord = (unsigned)(e & 0xFFFFFFFFull);
		const unsigned *pq = pref + q * (np + 1);
		int lo = 0, hi = np; // pq[lo] <= ord < pq[hi]: the rank whose list holds the ordinal
		while (hi - lo > 1) {
			const int mid = (lo + hi) >> 1;
			if (pq[mid] <= ord)
				lo = mid;
			else
				hi = mid;
		}
		const long long row = list_off[cI[q * np + lo]] + (ord - pq[lo]);
		const long long id = lids ? lids[row] : row;
		D[i] = pq_unkey((unsigned)(e >> 32), descending);
		I[i] = idmap ? idmap[id] : (lids ? id : id + id0);
	} else {
		D[i] = descending ? -FLT_MAX : FLT_MAX;
		I[i] = -1;
	}
}

} // namespace

// ---------------------------------------------------------------------------------------------- code store
void CodeStore::grow(int64_t need, int64_t ntotal, hipStream_t stream) {
	if (need <= cap)
		return;
	const int64_t nc = grown_cap(cap, need);
	mem.regrow((size_t)nc * pitch, (size_t)ntotal * pitch, true, stream);
	cap = nc;
}

// ---------------------------------------------------------------------------------------------- index
CodedListsIndex::CodedListsIndex(int kind_, int d_, int metric_, int64_t nlist_, int code_size_, size_t par_floats_, bool window_one_rank_,
                                 const Names &names_)
    : IndexBase(kind_, d_, metric_), names(names_), nlist(nlist_ > 0 ? nlist_ : 1), code_size(code_size_), par_floats(par_floats_), store(code_size_),
      dir(nlist), window_one_rank(window_one_rank_) {
	if (metric != METRIC_L2 && metric != METRIC_IP)
		throw_faiss(names.cls, names.file, "metric type %d is not implemented on the MI355X path", metric);
	if (nlist_ > 0) {
		coarse.nlist = nlist;
		coarse.quantizer.reset(new FlatIndex(d, metric));
	}
	is_trained = false;
}
CodedListsIndex::~CodedListsIndex() {
	(void)hipSetDevice(device);
	if (stream)
		(void)hipStreamSynchronize(stream);
}
void CodedListsIndex::free_device() { // the index leaves its device (to_device): load_image builds all of it again
	par_.release();
	h_flag.release();
	store.release();
	release_all();
	selector.release();
	recon_tab.drop();
	dirty = cent_dirty = true;
}
void CodedListsIndex::adopt_tuning(const Tuning &t) {
	tune_ = t;
	if (coarse)
		coarse.adopt_tuning(t);
}

// ------------------------------------------------------------------------------------------ coarse side, parameters
void CodedListsIndex::update_trained() {
	is_trained = have_par && (!coarse || coarse.quantizer->ntotal == nlist);
}
void CodedListsIndex::ensure_par() {
	if (!par_)
		par_ = DevBlock<float>(par_floats);
}
void CodedListsIndex::set_coarse(const float *c) {
	use_device();
	check_empty_for_training();
	coarse.set_centroids(c);
	cent_dirty = true;
	update_trained();
}
const float *CodedListsIndex::centroids_dev() {
	if (!coarse)
		return nullptr;
	if (cent_dirty) {
		std::vector<float> c((size_t)nlist * d);
		coarse.get_centroids(c.data());
		cent_dev.reserve(c.size() * sizeof(float));
		MVS_HIP(hipMemcpyAsync(cent_dev.p, c.data(), c.size() * sizeof(float), hipMemcpyHostToDevice, stream));
		MVS_HIP(hipStreamSynchronize(stream));
		cent_dirty = false;
	}
	return (const float *)cent_dev.p;
}
void CodedListsIndex::assign_device(int64_t n, const float *d_x, float *d_D, int64_t *d_I) {
	coarse.assign(n, d_x, d_D, d_I, stream);
	use_device();
}
void CodedListsIndex::train_coarse(int64_t n, const float *x) { // (niter 10, spherical under inner product: what IVF<n>,Flat runs)
	std::vector<float> cent((size_t)nlist * d);
	{
		CtorDevice scope(device);
		FlatIndex assigner(d, metric);
		assigner.adopt_tuning(tune_);
		kmeans_train({nlist, 10, metric == METRIC_IP}, n, x, assigner);
		assigner.copy_rows_to_host(cent.data());
	}
	have_par = false;
	set_coarse(cent.data());
}

// ------------------------------------------------------------------------------------------ add
void CodedListsIndex::set_label_offset(int64_t off) {
	if (coarse && ntotal > 0 && off != label_offset)
		throw_faiss((std::string(names.cls) + "::set_label_offset").c_str(), names.file, "the label offset of an IVF index must be set before rows are added");
	label_offset = off;
}
void CodedListsIndex::check_trained_for_add() const {
	if (!is_trained)
		throw_faiss(names.add_fn, names.add_file, "Error: 'is_trained' failed");
}
void CodedListsIndex::check_rows(int64_t n) const {
	if (n > (int64_t)0x7fffffff - 1024)
		throw_faiss((std::string(names.cls) + "::add").c_str(), names.file, "a single-device index holds at most 2^31 rows");
}
// d_x: [n][d] rows on the device, in `stream` order; ids (host) may be null
void CodedListsIndex::add_core_device(int64_t n, const float *d_x, const int64_t *ids_host) {
	check_trained_for_add();
	check_rows(ntotal + n);
	store.grow(ntotal + n, ntotal, stream);
	const int64_t bs = 65536; // IndexIVF::add_with_ids block size
	std::vector<int64_t> lab;
	if (coarse) {
		ws_lab.reserve((size_t)std::min(bs, n) * (sizeof(float) + sizeof(int64_t)));
		lab.resize((size_t)std::min(bs, n));
		dir.reserve(ntotal + n);
	}
	for (int64_t i0 = 0; i0 < n; i0 += bs) {
		const int64_t nb = std::min(bs, n - i0);
		int64_t *d_lab = nullptr;
		if (coarse) {
			d_lab = (int64_t *)ws_lab.p;
			assign_device(nb, d_x + i0 * d, (float *)(d_lab + nb), d_lab);
			MVS_HIP(hipMemcpyAsync(lab.data(), d_lab, (size_t)nb * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
		}
		encode_block(nb, d_x + i0 * d, d_lab, ntotal + i0);
		MVS_HIP(hipGetLastError());
		MVS_HIP(hipStreamSynchronize(stream));
		if (coarse)
			dir.append(nb, lab.data(), ids_host ? ids_host + i0 : nullptr, label_offset + ntotal + i0);
	}
	ntotal += n;
	dirty = true;
	recon_tab.drop();
}
void CodedListsIndex::add_host(int64_t n, const float *x, const int64_t *ids) {
	use_device();
	if (n <= 0)
		return;
	check_trained_for_add(); // (before the rows travel)
	const int64_t bs = 1 << 20; // rows staged at a time (a multiple of add_core_device's blocks): databases are larger than a staging buffer should be
	ws_add.reserve((size_t)std::min(bs, n) * d * sizeof(float));
	for (int64_t i0 = 0; i0 < n; i0 += bs) {
		const int64_t nb = std::min(bs, n - i0);
		MVS_HIP(hipMemcpyAsync(ws_add.p, x + i0 * d, (size_t)nb * d * sizeof(float), hipMemcpyHostToDevice, stream));
		add_core_device(nb, (const float *)ws_add.p, ids ? ids + i0 : nullptr);
	}
}
void CodedListsIndex::add(int64_t n, const float *x) {
	add_host(n, x, nullptr);
}
void CodedListsIndex::add_with_ids(int64_t n, const float *x, const int64_t *ids) {
	if (!coarse)
		return IndexBase::add_with_ids(n, x, ids); // "add_with_ids not implemented for this type of index"
	add_host(n, x, ids);
}
void CodedListsIndex::add_device(int64_t n, const float *d_x, hipStream_t st) {
	use_device();
	if (n <= 0)
		return;
	stream_wait(stream, st);
	add_core_device(n, d_x, nullptr);
}
void CodedListsIndex::add_with_ids_device(int64_t n, const float *d_x, const int64_t *d_ids, hipStream_t st) {
	if (!coarse)
		return IndexBase::add_with_ids_device(n, d_x, d_ids, st);
	use_device();
	if (n <= 0)
		return;
	stream_wait(stream, st);
	std::vector<int64_t> ids((size_t)n);
	MVS_HIP(hipMemcpy(ids.data(), d_ids, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
	add_core_device(n, d_x, ids.data());
}

// rows left, or arrived behind add()'s back (remove_ids; merge_from and copy_subset_to, csrc/merge.hip): the list view and the lookup table are derived again
void CodedListsIndex::lists_changed() {
	dirty = true;
	recon_tab.drop();
	sid_h.clear();
	top_rows.clear();
	max_list = nsorted = 0;
}

// ------------------------------------------------------------------------------------------ remove_ids
// Without a quantiser (SQ8): IndexFlatCodes::remove_ids, a stable compaction of the arrival-order store.  With one: IndexIVF::remove_ids,
// every list's swap-from-the-end loop on the host (csrc/remove_plan.h), the store gathered into the new list-major arrival order.  The
// list view is derived: dirty
int64_t CodedListsIndex::remove_ids(const mvs_search_params *sel, const int64_t *d_idmap, RemoveMarks *marks) {
	use_device();
	check_remove_selector(sel);
	if (ntotal <= 0)
		return 0;
	int64_t removed = 0;
	if (!coarse) {
		RemoveMarks own;
		RemoveMarks &m = marks ? *marks : own;
		const int64_t nkeep = remove_mark(m, selector.upload(sel, IdDomain::rows(label_offset, ntotal, d_idmap), stream), d_idmap, label_offset, ntotal, stream);
		if (nkeep == ntotal)
			return 0;
		store.compact(m, stream);
		removed = ntotal - nkeep;
		ntotal = nkeep;
	} else {
		IvfRemovePlan plan;
		if (!ivf_remove_plan_host(dir, sel, d_idmap, marks, plan, stream))
			return 0;
		store.gather(plan.perm, stream);
		removed = plan.removed;
		dir.adopt(std::move(plan));
		ntotal = dir.rows();
	}
	lists_changed();
	return removed;
}

// ------------------------------------------------------------------------------------------ list view
// rows grouped by list, arrival order inside a list (ArrayInvertedLists semantics), codes gathered on the device.
// Without a quantiser: one list = the arrival-order store
void CodedListsIndex::build_lists() {
	if (!dirty)
		return;
	if (!coarse) {
		list_off.assign((size_t)nlist + 1, 0);
		list_off[1] = ntotal;
		max_list = nsorted = ntotal;
		top_rows.assign(1, ntotal);
	} else {
		ListDirectory::Groups g = dir.group();
		sid_h = dir.sorted_ids(g);
		const std::vector<int32_t> &perm = g.perm;
		list_off.swap(g.off);
		nsorted = list_off[(size_t)nlist];
		max_list = 0;
		top_rows.assign((size_t)nlist, 0);
		for (int64_t l = 0; l < nlist; l++) {
			top_rows[(size_t)l] = list_off[(size_t)l + 1] - list_off[(size_t)l];
			max_list = std::max(max_list, top_rows[(size_t)l]);
		}
		std::sort(top_rows.begin(), top_rows.end(), std::greater<int64_t>());
		for (int64_t l = 1; l < nlist; l++)
			top_rows[(size_t)l] += top_rows[(size_t)l - 1];
		lcodes.reserve((size_t)std::max<int64_t>(nsorted, 1) * store.pitch);
		lids.reserve((size_t)std::max<int64_t>(nsorted, 1) * sizeof(int64_t));
		DevBuf dperm;
		dperm.reserve((size_t)std::max<int64_t>(nsorted, 1) * sizeof(int32_t));
		if (nsorted > 0) {
			MVS_HIP(hipMemcpyAsync(dperm.p, perm.data(), (size_t)nsorted * sizeof(int32_t), hipMemcpyHostToDevice, stream));
			MVS_HIP(hipMemcpyAsync(lids.p, sid_h.data(), (size_t)nsorted * sizeof(int64_t), hipMemcpyHostToDevice, stream));
			const int words = store.pitch / 16;
			const long long tot = nsorted * words;
			hipLaunchKernelGGL(coded_gather_codes_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, (const uint4 *)store.codes(),
			                   (const int *)dperm.p, (long long)nsorted, words, (uint4 *)lcodes.p);
			MVS_HIP(hipGetLastError());
		}
		MVS_HIP(hipStreamSynchronize(stream)); // (dperm is released)
	}
	list_off_dev.reserve(list_off.size() * sizeof(int64_t));
	MVS_HIP(hipMemcpyAsync(list_off_dev.p, list_off.data(), list_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
	MVS_HIP(hipStreamSynchronize(stream));
	dirty = false;
}
const unsigned char *CodedListsIndex::list_codes() const {
	return coarse ? (const unsigned char *)lcodes.p : store.codes();
}
int64_t CodedListsIndex::list_size(int64_t l) {
	use_device();
	if (l < 0 || l >= nlist)
		throw_faiss((std::string(names.cls) + "::list_size").c_str(), names.file, "list %lld is outside [0, %lld)", (long long)l, (long long)nlist);
	build_lists();
	return list_off[(size_t)l + 1] - list_off[(size_t)l];
}
void CodedListsIndex::get_list(int64_t l, int64_t *ids, uint8_t *codes) {
	const int64_t n = list_size(l), b = list_off[(size_t)l];
	if (n <= 0)
		return;
	if (ids)
		memcpy(ids, &sid_h[(size_t)b], (size_t)n * sizeof(int64_t));
	if (codes)
		MVS_HIP(hipMemcpy2D(codes, (size_t)code_size, list_codes() + (size_t)b * store.pitch, (size_t)store.pitch, (size_t)code_size, (size_t)n,
		                    hipMemcpyDeviceToHost));
}

// ------------------------------------------------------------------------------------------ search
// the rows one query can send to its bucket from a unit, at most
int64_t CodedListsIndex::unit_rows(int ra, int rb, int64_t p0, int64_t p1) const {
	if (rb - ra == 1)
		return std::min(max_list, p1) - p0;
	return top_rows[(size_t)std::min<int64_t>(rb - ra, nlist) - 1];
}
void CodedListsIndex::launch_scan(Chunk &c, int ra, int rb, int64_t p0, int64_t p1) {
	const int Q = c.Q, span = rb - ra;
	const int64_t npairs = c.nqc * span;
	// the unit's pairs grouped by list: count, offsets, scatter
	MVS_HIP(hipMemsetAsync(c.gcnt, 0, (size_t)2 * nlist * sizeof(int), stream));
	const dim3 pgrid((unsigned)((npairs + 255) / 256));
	hipLaunchKernelGGL(coded_count_kernel, pgrid, dim3(256), 0, stream, (const long long *)c.cI, (long long)c.nqc, c.np, ra, rb,
	                   (const long long *)list_off_dev.p, (long long)nlist, (long long)p0, c.gcnt);
	hipLaunchKernelGGL(coded_offsets_kernel, dim3(1), dim3(1024), 0, stream, (const int *)c.gcnt, (int)nlist, Q, c.poff, c.goff);
	hipLaunchKernelGGL(coded_scatter_kernel, pgrid, dim3(256), 0, stream, (const long long *)c.cI, (long long)c.nqc, c.np, ra, rb,
	                   (const long long *)list_off_dev.p, (long long)nlist, (long long)p0, (const int *)c.poff, c.gcur, (int2 *)ws_pairs.p);
	MVS_HIP(hipGetLastError());
	// pair groups: sum over lists of ceil(pairs / Q) <= pairs / Q + lists that have pairs; segments of R positions of the window
	const int64_t gx = npairs / Q + 1 + std::min<int64_t>(nlist, npairs);
	const int64_t gy = (std::min(max_list, p1) - p0 + ROWS_PER_WG - 1) / ROWS_PER_WG;
	c.a.p0 = p0, c.a.p1 = p1;
	begin_kernel_timing(stream);
	launch_scan_kernel(c.a, dim3((unsigned)gx, (unsigned)gy), c.nqc, (double)unit_rows(ra, rb, p0, p1));
	MVS_HIP(hipGetLastError());
	end_kernel_timing(stream);
	++last_launches;
}
// ranks [ra, rb), positions [p0, p1) of their lists, into every list of the chunk
void CodedListsIndex::scan_unit(Chunk &c, int ra, int rb, int64_t p0, int64_t p1) {
	launch_scan(c, ra, rb, p0, p1);
	if (unit_rows(ra, rb, p0, p1) > ROWS_PER_WG) { // (a unit of at most R rows per query cannot overflow a bucket of R entries)
		MVS_HIP(hipMemcpyAsync(h_flag.p, c.a.overflow, sizeof(int), hipMemcpyDeviceToHost, stream));
		MVS_HIP(hipStreamSynchronize(stream));
		if (*(const int *)h_flag.p) { // some bucket overflowed: nothing of this unit is merged; its two halves one after the other
			MVS_HIP(hipMemsetAsync(c.a.cnt, 0, (size_t)c.nqc * sizeof(unsigned), stream));
			MVS_HIP(hipMemsetAsync(c.a.overflow, 0, sizeof(int), stream));
			++last_rescans;
			if (rb - ra > 1) {
				const int mid = ra + (rb - ra) / 2;
				scan_unit(c, ra, mid, p0, p1);
				scan_unit(c, mid, rb, p0, p1);
			} else {
				const int64_t w1 = std::min(max_list, p1);
				const int64_t mid = p0 + ((w1 - p0) / 2 + ROWS_PER_WG - 1) / ROWS_PER_WG * ROWS_PER_WG;
				scan_unit(c, ra, rb, p0, mid);
				scan_unit(c, ra, rb, mid, w1);
			}
			return;
		}
	}
	int P = 1;
	while (P < c.k + ROWS_PER_WG)
		P <<= 1;
	const size_t lds = (size_t)P * sizeof(unsigned long long);
	ensure_dynamic_lds((const void *)pq_select_kernel, lds);
	hipLaunchKernelGGL(pq_select_kernel, dim3((unsigned)c.nqc), dim3(1024), lds, stream, c.list, c.len, c.k, (const unsigned long long *)c.a.bucket,
	                   c.a.cnt, const_cast<unsigned *>(c.a.thr));
	MVS_HIP(hipGetLastError());
}
void CodedListsIndex::search_mapped(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params,
                                    const int64_t *d_idmap, hipStream_t st) {
	use_device();
	const char *fn = coarse ? "virtual void faiss::IndexIVF::search(...) const" : "virtual void faiss::IndexFlatCodes::search(...) const";
	const char *file = coarse ? "faiss/IndexIVF.cpp" : "faiss/IndexFlatCodes.cpp";
	if (k <= 0)
		throw_faiss(fn, file, "Error: 'k > 0' failed");
	if (k > PQ_MAX_K)
		throw_faiss((std::string(names.cls) + "::search").c_str(), names.file,
		            "k = %lld is beyond the largest k the %s index serves on the MI355X path (%d)", (long long)k, names.label, PQ_MAX_K);
	if (!is_trained)
		throw_faiss(fn, file, "Error: 'is_trained' failed");
	if (nq <= 0)
		return;
	int64_t np = 1;
	if (coarse) {
		np = params && params->nprobe > 0 ? params->nprobe : nprobe;
		np = std::min(np, nlist); // IndexIVF::search: nprobe = min(nlist, params->nprobe)
		if (np <= 0)
			throw_faiss(fn, file, "Error: 'nprobe > 0' failed");
	}
	stream_wait(stream, st); // our stream carries the adds and the list view; the caller's the queries
	build_lists();
	const float *d_cent = centroids_dev();
	const int Q = pair_block();
	// 1. the probed lists of the whole batch (no quantiser: list 0 at rank 0), the ordinal bases
	ws_cI.reserve((size_t)nq * np * sizeof(int64_t));
	ws_pref.reserve((size_t)nq * (np + 1) * sizeof(unsigned));
	if (nsorted > 0) {
		if (coarse) {
			ws_cD.reserve((size_t)nq * np * sizeof(float));
			coarse.topk(nq, d_x, np, (float *)ws_cD.p, (int64_t *)ws_cI.p, nullptr, stream);
			use_device();
		} else {
			MVS_HIP(hipMemsetAsync(ws_cI.p, 0, (size_t)nq * sizeof(int64_t), stream));
		}
		hipLaunchKernelGGL(coded_prefix_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, (const long long *)ws_cI.p, (long long)nq,
		                   (int)np, (const long long *)list_off_dev.p, (long long)nlist, (unsigned *)ws_pref.p);
		MVS_HIP(hipGetLastError());
	}
	// 2. queries per chunk: buckets <= 256 MB
	const int64_t nqc_max = std::min<int64_t>(nq, (int64_t)(PQ_BUCKET_SCRATCH / ((size_t)ROWS_PER_WG * sizeof(unsigned long long))));
	int np_span = 1; // the widest rank span a unit can have
	for (int ra = 0, rb = 1; ra < np; ra = rb, rb = (int)std::min<int64_t>(np, 3 * (int64_t)rb))
		np_span = std::max(np_span, rb - ra);
	ws_bucket.reserve((size_t)nqc_max * ROWS_PER_WG * sizeof(unsigned long long));
	ws_list.reserve((size_t)nqc_max * k * sizeof(unsigned long long));
	ws_pairs.reserve((size_t)nqc_max * np_span * sizeof(int2));
	ws_grp.reserve((size_t)(4 * nlist + 2) * sizeof(int)); // cnt [nlist] | cur [nlist] | poff [nlist + 1] | goff [nlist + 1]
	// control block: len [nqc] | cnt [nqc] | overflow (+ pad) | thr [nqc]
	const size_t ctl_zero = (size_t)(2 * nqc_max + 4) * sizeof(int);
	ws_ctl.reserve(ctl_zero + (size_t)nqc_max * sizeof(unsigned));
	h_flag.reserve(sizeof(int));
	Chunk c;
	c.k = (int)k, c.Q = Q, c.np = (int)np;
	c.list = (unsigned long long *)ws_list.p;
	c.len = (int *)ws_ctl.p;
	c.gcnt = (int *)ws_grp.p;
	c.gcur = c.gcnt + nlist;
	c.poff = c.gcur + nlist;
	c.goff = c.poff + nlist + 1;
	CodedScan &a = c.a;
	a.codes = list_codes();
	a.lids = coarse ? (const long long *)lids.p : nullptr;
	a.list_off = (const long long *)list_off_dev.p;
	a.cent = d_cent;
	a.par = d_par();
	a.pairs = (const int2 *)ws_pairs.p;
	a.poff = c.poff, a.goff = c.goff;
	a.bucket = (unsigned long long *)ws_bucket.p;
	a.cnt = (unsigned *)ws_ctl.p + nqc_max;
	a.overflow = (int *)ws_ctl.p + 2 * nqc_max;
	a.thr = (unsigned *)((char *)ws_ctl.p + ctl_zero);
	a.idmap = (const long long *)d_idmap;
	a.id0 = label_offset;
	a.nlist = (int)nlist, a.d = d, a.pitch = store.pitch, a.np = (int)np;
	a.p0 = 0, a.p1 = 0;
	// (the scans test the stored id of a list entry, or label_offset + row without lists; under an id map, its entry there)
	a.sel = selector.upload(params, coarse ? IdDomain::ids((const int64_t *)lids.p, nsorted, d_idmap) : IdDomain::rows(label_offset, ntotal, d_idmap), stream);
	last_launches = last_rescans = 0;
	memset(&kinfo, 0, sizeof kinfo);
	for (int64_t q0 = 0; q0 < nq; q0 += nqc_max) {
		c.nqc = std::min(nqc_max, nq - q0);
		c.cI = (const int64_t *)ws_cI.p + q0 * np;
		a.xq = d_x + q0 * d;
		a.pref = (const unsigned *)ws_pref.p + q0 * (np + 1);
		MVS_HIP(hipMemsetAsync(ws_ctl.p, 0, ctl_zero, stream));
		pq_open_bounds(const_cast<unsigned *>(a.thr), (size_t)nqc_max, stream); // (an open list admits what FAISS's neutral-filled heap admits: csrc/pq_kernels.h)
		if (nsorted > 0)
			for (int ra = 0, rb = 1; ra < np; ra = rb, rb = (int)std::min<int64_t>(np, 3 * (int64_t)rb)) {
				if (rb - ra > 1 || !window_one_rank) {
					scan_unit(c, ra, rb, 0, max_list);
					continue;
				}
				// one rank: windows [0, R), [R, 3R), [3R, 9R), ... -- positions ascend, so the ordinals still do
				for (int64_t p0 = 0, p1 = ROWS_PER_WG; p0 < max_list; p0 = p1, p1 = 3 * p1)
					scan_unit(c, ra, rb, p0, std::min(p1, max_list));
			}
		const int64_t tot = c.nqc * k;
		hipLaunchKernelGGL(coded_emit_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, (const unsigned long long *)c.list,
		                   (const int *)c.len, c.k, (long long)c.nqc, metric == METRIC_IP ? 1 : 0, (const long long *)c.cI, (int)np, a.pref,
		                   (const long long *)list_off_dev.p, a.lids, (long long)label_offset,
		                   raw_labels ? nullptr : (const long long *)d_idmap, d_D + q0 * k, // (raw_labels: csrc/index.h; the offset of a refine base stays 0)
		                   (long long *)(d_I + q0 * k));
		MVS_HIP(hipGetLastError());
	}
	stream_wait(st, stream);
}
void CodedListsIndex::search_device(int64_t nq, const float *d_x, int64_t k, float *d_D, int64_t *d_I, const mvs_search_params *params, hipStream_t st) {
	search_mapped(nq, d_x, k, d_D, d_I, params, nullptr, st);
}
bool CodedListsIndex::named_stat(const char *name, int64_t *value) {
	const size_t np = strlen(names.stat);
	if (strncmp(name, names.stat, np) != 0)
		return false;
	name += np;
	if (!strcmp(name, "_pair_block"))
		*value = pair_block();
	else if (!strcmp(name, "_rows_per_workgroup"))
		*value = ROWS_PER_WG;
	else if (!strcmp(name, "_scan_launches"))
		*value = last_launches;
	else if (!strcmp(name, "_scan_rescans"))
		*value = last_rescans;
	else
		return false;
	return true;
}
size_t CodedListsIndex::device_bytes() const {
	return (size_t)store.cap * store.pitch + lcodes.cap + lids.cap + (d_par() ? par_floats * sizeof(float) : 0);
}

// ------------------------------------------------------------------------------------------ images, placement
// no quantiser: codes [ntotal][code_size]; else the ArrayInvertedLists image, per list code_size-byte codes and ids in arrival order
void CodedListsIndex::to_host(HostIndex &out) {
	use_device();
	MVS_HIP(hipStreamSynchronize(stream));
	out.kind = kind;
	out.d = d;
	out.metric = metric;
	out.metric_arg = metric_arg;
	out.ntotal = ntotal;
	out.is_trained = is_trained;
	params_to_host(out);
	const size_t cs = (size_t)code_size;
	std::vector<uint8_t> all((size_t)ntotal * cs); // the arrival-order store
	if (ntotal > 0)
		MVS_HIP(hipMemcpy2D(all.data(), cs, store.codes(), (size_t)store.pitch, cs, (size_t)ntotal, hipMemcpyDeviceToHost));
	if (!coarse) {
		(out.*names.flat).swap(all);
		return;
	}
	out.nlist = nlist;
	out.nprobe = nprobe;
	coarse.to_host(out);
	std::vector<std::vector<int32_t>> list_pos;
	dir.to_lists(out.list_ids, list_pos);
	out.list_bytes.assign((size_t)nlist, {});
	for (int64_t l = 0; l < nlist; l++) {
		auto &c = out.list_bytes[(size_t)l];
		for (int32_t i : list_pos[(size_t)l])
			c.insert(c.end(), &all[(size_t)i * cs], &all[(size_t)i * cs] + cs);
	}
}
// rows of an inverted-lists image enter in list order, which keeps the arrival order inside every list
void CodedListsIndex::load_image(const HostIndex &h) {
	const size_t cs = (size_t)code_size;
	check_image(h);
	int64_t n = h.ntotal;
	if (coarse) {
		n = 0;
		for (int64_t l = 0; l < nlist; l++) {
			if (h.list_bytes[(size_t)l].size() != h.list_ids[(size_t)l].size() * cs)
				throw_faiss("faiss::Index* faiss::read_index(...)", "faiss/impl/index_read.cpp", "%s image: list %lld holds %zu code bytes for %zu ids",
				            names.image, (long long)l, h.list_bytes[(size_t)l].size(), h.list_ids[(size_t)l].size());
			n += (int64_t)h.list_ids[(size_t)l].size();
		}
	}
	check_rows(n);
	use_device();
	metric_arg = h.metric_arg;
	nprobe = h.nprobe;
	params_from_host(h);
	cent_dirty = true;
	update_trained();
	store.grow(n, ntotal, stream);
	std::vector<uint8_t> all;
	const uint8_t *src = nullptr;
	if (coarse) {
		dir.adopt_image(h.list_ids);
		all.reserve((size_t)n * cs);
		for (int64_t l = 0; l < nlist; l++)
			all.insert(all.end(), h.list_bytes[(size_t)l].begin(), h.list_bytes[(size_t)l].end());
		src = all.data();
	} else {
		src = (h.*names.flat).data();
	}
	if (n > 0)
		MVS_HIP(hipMemcpy2D(store.codes(), (size_t)store.pitch, src, cs, cs, (size_t)n, hipMemcpyHostToDevice));
	ntotal = n;
	dirty = true;
	recon_tab.drop();
}
void CodedListsIndex::to_device(int new_device) {
	if (new_device == device)
		return;
	check_device(new_device);
	HostIndex img;
	to_host(img);
	use_device();
	MVS_HIP(hipStreamSynchronize(stream));
	free_device();
	have_par = false;
	move_stream(new_device);
	if (coarse)
		coarse.quantizer->to_device(new_device);
	ntotal = 0;
	load_image(img);
}
IndexBase *CodedListsIndex::clone(int on_device) {
	check_device(on_device);
	HostIndex img;
	to_host(img);
	IndexBase *c = index_from_host(img, on_device); // (the kind's *_from_host)
	c->label_offset = label_offset;
	return c;
}

CodedListsIndex *coded_lists_of(IndexBase *ix) {
	return ix && (ix->kind == MVS_KIND_IVFPQ || ix->kind == MVS_KIND_SQ || ix->kind == MVS_KIND_IVFSQ) ? static_cast<CodedListsIndex *>(ix) : nullptr;
}

} // namespace mvs
