// csrc/merge.hip -- merge_from, check_compatible_for_merge and copy_subset_to (include/mi355_faiss.h "merge_from and copy_subset_to";
// DESIGN.md 3.18): the device side and the host code of the kinds whose classes live in headers (Flat, IDMap, the coded lists); "PQ<M>"
// and "IVF<n>,Flat" add theirs in csrc/pq.hip and csrc/ivf.hip.  Rows move from one index's append-only store to the tail of another's,
// device to device; an IVF kind's host directory is appended (csrc/list_directory.h) and its list views are derived again on demand.
// Every allocation that can fail is made before anything changes.
//
// Kernels
//   merge_flat_rows_kernel   Flat f32 rows and their norms, one lane per group of four floats (16-byte loads and stores), grid-stride.  In
//                            the pair-interleaved layout the place of a float inside its group depends on bit 4 of the ROW NUMBER
//                            ([k0,k2,k1,k3] clear, [k1,k3,k0,k2] set): a row whose new number has the other bit 4 gets the halves of every
//                            group swapped on the way.  CONVERT = false is the plain copy: plain row-major rows, or a destination offset that
//                            keeps every row's phase (a multiple of 32 rows)
//   merge_append_rows_kernel rows of `pitch` bytes as uint4 to the tail of another store: row i, or row pos[i] (copy_subset_to)
//   merge_append_ids_kernel  dst[i] = src[i] + add_id: the id map of IDMap
//   merge_equal_kernel       two arrays word by word; a difference raises one flag word (centroids, codebooks, ranges: compared where they live)
#include "coded_lists.h"

#include <chrono>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <typeinfo>

namespace mvs {

namespace {

constexpr long long MAX_BLOCKS = 1 << 20; // (grid-stride loops: a grid never exceeds this)

unsigned grid_for(long long total) {
	return (unsigned)std::max<long long>(1, std::min<long long>((total + 255) / 256, MAX_BLOCKS));
}

template <bool CONVERT>
__global__ __launch_bounds__(256) void merge_flat_rows_kernel(const float4 *__restrict__ src, const float *__restrict__ src_norms, long long src_row0,
                                                              long long n, int cpr, float4 *__restrict__ dst, float *__restrict__ dst_norms,
                                                              long long dst_row0) {
	const long long total = n * cpr;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const long long r = i / cpr;
		const int g = (int)(i - r * cpr);
		const long long rs = src_row0 + r, rd = dst_row0 + r;
		float4 v = src[rs * cpr + g];
		if (CONVERT && (((rs ^ rd) >> 4) & 1)) // [k0,k2,k1,k3] <-> [k1,k3,k0,k2]: the halves change places
			v = make_float4(v.z, v.w, v.x, v.y);
		dst[rd * cpr + g] = v;
		if (g == 0)
			dst_norms[rd] = src_norms[rs];
	}
}

__global__ __launch_bounds__(256) void merge_append_rows_kernel(const uint4 *__restrict__ src, const long long *__restrict__ pos, long long n, int words,
                                                                uint4 *__restrict__ dst) {
	const long long total = n * words;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		if (!pos) { // (contiguous: the items are the source's words in order)
			dst[i] = src[i];
			continue;
		}
		const long long r = i / words;
		const int w = (int)(i - r * words);
		dst[i] = src[pos[r] * words + w];
	}
}

__global__ __launch_bounds__(256) void merge_append_ids_kernel(const long long *__restrict__ src, long long n, long long add_id, long long *__restrict__ dst) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
		dst[i] = src[i] + add_id;
}

__global__ __launch_bounds__(256) void merge_equal_kernel(const unsigned *__restrict__ a, const unsigned *__restrict__ b, long long nwords,
                                                          unsigned *__restrict__ differ) {
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (long long)gridDim.x * blockDim.x)
		if (a[i] != b[i])
			*differ = 1u; // (every writer stores the same word)
}

} // namespace

void merge_refuse_add_id() {
	throw_faiss("virtual void faiss::IndexFlatCodes::merge_from(faiss::Index&, faiss::idx_t)", "faiss/IndexFlatCodes.cpp", "cannot set ids in FlatCodes index");
}

// ---------------------------------------------------------------------------------------------- launchers
void launch_merge_flat_rows(const FlatGeom &g, const float *d_src, const float *d_src_norms, int64_t src_row0, int64_t n, float *d_dst,
                            float *d_dst_norms, int64_t dst_row0, hipStream_t st) {
	if (n <= 0)
		return;
	const int cpr = g.dp / 4;
	const bool convert = g.pair_interleaved && ((dst_row0 - src_row0) & 31) != 0;
	const dim3 grid(grid_for((long long)n * cpr));
	if (convert)
		hipLaunchKernelGGL(merge_flat_rows_kernel<true>, grid, dim3(256), 0, st, (const float4 *)d_src, d_src_norms, (long long)src_row0, (long long)n, cpr,
		                   (float4 *)d_dst, d_dst_norms, (long long)dst_row0);
	else
		hipLaunchKernelGGL(merge_flat_rows_kernel<false>, grid, dim3(256), 0, st, (const float4 *)d_src, d_src_norms, (long long)src_row0, (long long)n, cpr,
		                   (float4 *)d_dst, d_dst_norms, (long long)dst_row0);
	MVS_HIP(hipGetLastError());
}

void launch_merge_append_rows(const void *d_src, const int64_t *d_pos, int64_t n, int pitch, void *d_dst, int64_t dst_row0, hipStream_t st) {
	if (n <= 0)
		return;
	const int words = pitch / 16;
	hipLaunchKernelGGL(merge_append_rows_kernel, dim3(grid_for((long long)n * words)), dim3(256), 0, st, (const uint4 *)d_src, (const long long *)d_pos,
	                   (long long)n, words, (uint4 *)((unsigned char *)d_dst + (size_t)dst_row0 * pitch));
	MVS_HIP(hipGetLastError());
}

void launch_merge_append_ids(const int64_t *d_src, int64_t n, int64_t add_id, int64_t *d_dst, hipStream_t st) {
	if (n <= 0)
		return;
	hipLaunchKernelGGL(merge_append_ids_kernel, dim3(grid_for(n)), dim3(256), 0, st, (const long long *)d_src, (long long)n, (long long)add_id,
	                   (long long *)d_dst);
	MVS_HIP(hipGetLastError());
}

bool merge_dev_equal(const void *d_a, const void *d_b, size_t bytes, hipStream_t st) {
	if (bytes == 0 || d_a == d_b)
		return true;
	DevBuf flag;
	flag.reserve(sizeof(unsigned));
	MVS_HIP(hipMemsetAsync(flag.p, 0, sizeof(unsigned), st));
	const long long nwords = (long long)(bytes / sizeof(unsigned)); // (f32 arrays: whole words)
	hipLaunchKernelGGL(merge_equal_kernel, dim3(grid_for(nwords)), dim3(256), 0, st, (const unsigned *)d_a, (const unsigned *)d_b, nwords, (unsigned *)flag.p);
	MVS_HIP(hipGetLastError());
	unsigned differ = 0;
	MVS_HIP(hipMemcpyAsync(&differ, flag.p, sizeof differ, hipMemcpyDeviceToHost, st));
	MVS_HIP(hipStreamSynchronize(st));
	return differ == 0;
}

// ---------------------------------------------------------------------------------------------- the checks every kind shares
void merge_refuse(const char *fmt, ...) {
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	throw_faiss("virtual void faiss::Index::check_compatible_for_merge(const faiss::Index&) const", "faiss/Index.cpp", "check_compatible_for_merge: %s", buf);
}
void merge_check_common(IndexBase &a, IndexBase &b) {
	if (&a == &b)
		merge_refuse("other == this: an index cannot be merged into itself");
	if (is_sharded(&a) || is_sharded(&b))
		merge_refuse("a sharded index takes no part in a merge");
	if (a.kind != b.kind || typeid(a) != typeid(b))
		merge_refuse("the index kinds differ (kind %d against kind %d)", a.kind, b.kind);
	if (a.d != b.d)
		merge_refuse("d differs (%d against %d)", a.d, b.d);
	if (a.metric != b.metric || a.metric_arg != b.metric_arg)
		merge_refuse("the metric differs (%d against %d)", a.metric, b.metric);
	if (a.device != b.device)
		merge_refuse("the indexes live on different devices (%d against %d): merging across devices is not implemented", a.device, b.device);
}
void merge_check_coarse(IndexBase &a, CoarseSide &ca, IndexBase &b, CoarseSide &cb) {
	if (ca.nlist != cb.nlist)
		merge_refuse("nlist differs (%lld against %lld)", (long long)ca.nlist, (long long)cb.nlist);
	if (ca.quantizer->kind != cb.quantizer->kind)
		merge_refuse("the coarse quantizers differ in kind (%d against %d)", ca.quantizer->kind, cb.quantizer->kind);
	if (!a.is_trained || !b.is_trained)
		merge_refuse("%s is not trained", a.is_trained ? "the other index" : "this index");
	FlatIndex *fa = ca.flat(), *fb = cb.flat();
	bool same;
	if (fa && fb) { // rows 0 .. nlist-1 of two Flat stores of one geometry have the same layout: compared where they are
		fa->flush_adds(), fb->flush_adds();
		a.use_device();
		stream_wait(a.stream, fa->stream), stream_wait(a.stream, fb->stream);
		same = merge_dev_equal(fa->vecs(), fb->vecs(), (size_t)ca.nlist * fa->geom.dp * sizeof(float), a.stream);
	} else { // an HNSW quantiser keeps its centroids behind the graph: its image's rows (nlist * d floats) are compared
		std::vector<float> xa((size_t)ca.nlist * a.d), xb(xa.size());
		ca.get_centroids(xa.data()), cb.get_centroids(xb.data());
		a.use_device();
		same = memcmp(xa.data(), xb.data(), xa.size() * sizeof(float)) == 0;
	}
	if (!same)
		merge_refuse("the coarse centroids differ");
}
static double now_ms() {
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
MergeLaps::MergeLaps(const char *kind_) : kind(kind_), on(getenv("MVS_MERGE_PROFILE") != nullptr), t_prev_ms(on ? now_ms() : 0.0) {
}
void MergeLaps::lap(const char *what, hipStream_t st) {
	if (!on)
		return;
	(void)hipStreamSynchronize(st);
	const double t = now_ms();
	fprintf(stderr, "mergeprofile\t%s %s: %.3f ms\n", kind, what, t - t_prev_ms);
	t_prev_ms = t;
}
void merge_check_subset_type(int subset_type, int64_t a1) {
	if (subset_type < 0 || subset_type > 2)
		throw_faiss("faiss::InvertedLists::copy_subset_to", "faiss/invlists/InvertedLists.cpp", "subset type not implemented");
	if (subset_type == 1 && a1 <= 0)
		throw_faiss("faiss::InvertedLists::copy_subset_to", "faiss/invlists/InvertedLists.cpp", "copy_subset_to: SUBSET_TYPE_ID_MOD needs a1 > 0, not %lld", (long long)a1);
}

// ---------------------------------------------------------------------------------------------- the base refuses
void IndexBase::check_compatible_for_merge(IndexBase &) {
	throw_faiss("virtual void faiss::Index::check_compatible_for_merge(const faiss::Index&) const", "faiss/Index.cpp", "check_compatible_for_merge() not implemented");
}
void IndexBase::merge_from(IndexBase &, int64_t) {
	throw_faiss("virtual void faiss::Index::merge_from(faiss::Index&, faiss::idx_t)", "faiss/Index.cpp", "merge_from() not implemented");
}
void IndexBase::copy_subset_to(IndexBase &, int, int64_t, int64_t) {
	throw_faiss("virtual void faiss::IndexIVF::copy_subset_to(...) const", "faiss/IndexIVF.cpp", "copy_subset_to is implemented for the bare IVF kinds only");
}

// ---------------------------------------------------------------------------------------------- Flat
void FlatIndex::check_compatible_for_merge(IndexBase &other) {
	merge_check_common(*this, other);
}
// IndexFlatCodes::merge_from: other's row i becomes row ntotal + i.  The derived stores (bf16 hi/lo, h1, int8, the shadow clustering) cover
// rows [0, their n) and are extended before the next search that reads them, exactly as after add(); other is reset()
void FlatIndex::merge_from(IndexBase &other, int64_t add_id) {
	check_compatible_for_merge(other);
	if (add_id != 0)
		merge_refuse_add_id();
	FlatIndex &o = static_cast<FlatIndex &>(other);
	MergeLaps laps("Flat");
	const int64_t nb = o.ntotal;
	if (ntotal + nb > (int64_t)0x7fffffff - 1024)
		throw_faiss("mvs::FlatIndex::merge_from", __FILE__, "a single-device shard holds at most 2^31 rows");
	o.use_device();
	o.flush_adds(); // (staged rows reach the source's store on its stream)
	use_device();
	if (nb > 0) {
		flush_adds();
		// `stream` goes behind the source's stream and behind any search a caller's stream may still run on either store -- before the growth,
		// whose retirement of the old rows is an event on `stream`
		stream_wait(stream, o.stream);
		if (have_last_search)
			stream_wait(stream, last_search_stream);
		if (o.have_last_search)
			stream_wait(stream, o.last_search_stream);
		laps.lap("compatibility + staged rows", stream);
		grow(ntotal + nb, stream); // (before anything changes: a failure leaves both indexes as they were)
		laps.lap("growth allocation + copy of the old rows", stream);
		launch_merge_flat_rows(geom, o.vecs(), o.norms(), 0, nb, vecs(), norms(), ntotal, stream);
		MVS_HIP(hipStreamSynchronize(stream)); // (the source may be written again as soon as this returns)
		laps.lap("move kernel", stream);
		ntotal += nb;
	}
	o.reset();
	laps.lap("the source's reset (its derived stores go)", stream);
}

// ---------------------------------------------------------------------------------------------- IDMap
void IDMapIndex::check_compatible_for_merge(IndexBase &other) {
	merge_check_common(*this, other);
	IDMapIndex &o = static_cast<IDMapIndex &>(other);
	if (is_idmap2 != o.is_idmap2)
		merge_refuse("the index kinds differ (IDMap against IDMap2)");
	sub->check_compatible_for_merge(*o.sub);
}
// IndexIDMap::merge_from: the wrapped indexes merge, then other's id map + add_id follows this one's.  A wrapped IVF kind names its rows
// by stored id 0 .. ntotal-1 and labels are id_map[stored id]: other's stored ids are shifted by this sub-index's ntotal (FAISS passes 0
// -- include/mi355_faiss.h)
void IDMapIndex::merge_from(IndexBase &other, int64_t add_id) {
	check_compatible_for_merge(other);
	IDMapIndex &o = static_cast<IDMapIndex &>(other);
	o.use_device();
	o.flush_ids();
	use_device();
	flush_ids();
	const int64_t n0 = ntotal, nb = o.ntotal;
	grow_ids(n0 + nb, stream); // (before anything changes; synchronises)
	sub->merge_from(*o.sub, coarse_side_of(sub) ? sub->ntotal : 0);
	use_device();
	if (nb > 0) {
		stream_wait(stream, o.stream);
		launch_merge_append_ids(o.ids.get(), nb, add_id, ids.get() + n0, stream);
		MVS_HIP(hipStreamSynchronize(stream));
	}
	ntotal = sub->ntotal;
	recon_tab.drop();
	o.ntotal = o.sub->ntotal;
	o.recon_tab.drop();
}

// ---------------------------------------------------------------------------------------------- coded lists: IVF<n>,PQ<M>, IVF<n>,SQ8, SQ8
void CodedListsIndex::check_compatible_for_merge(IndexBase &other) {
	merge_check_common(*this, other);
	CodedListsIndex &o = static_cast<CodedListsIndex &>(other);
	if (code_size != o.code_size || par_floats != o.par_floats)
		merge_refuse("the code size differs (%d bytes against %d; M for a product quantizer)", code_size, o.code_size);
	if ((bool)coarse != (bool)o.coarse)
		merge_refuse("the index kinds differ (one has inverted lists)");
	if (coarse)
		merge_check_coarse(*this, coarse, o, o.coarse);
	if (!is_trained || !o.is_trained || !have_par || !o.have_par)
		merge_refuse("%s is not trained", is_trained && have_par ? "the other index" : "this index");
	use_device();
	stream_wait(stream, o.stream);
	if (!merge_dev_equal(d_par(), o.d_par(), par_floats * sizeof(float), stream))
		merge_refuse("the %s differ", kind == MVS_KIND_IVFPQ ? "PQ codebooks" : "SQ ranges");
}
// IndexIVF::merge_from (a quantiser) / IndexFlatCodes::merge_from ("SQ8"): other's code rows follow this store's, byte for byte; with a
// quantiser other's directory follows this one's with its stored ids + add_id.  Other keeps parameters and centroids and gives up its store
void CodedListsIndex::merge_from(IndexBase &other, int64_t add_id) {
	check_compatible_for_merge(other);
	if (!coarse && add_id != 0)
		merge_refuse_add_id();
	CodedListsIndex &o = static_cast<CodedListsIndex &>(other);
	use_device();
	MergeLaps laps(names.image);
	const int64_t nb = o.ntotal;
	check_rows(ntotal + nb);
	if (nb > 0) {
		laps.lap("compatibility", stream);
		store.grow(ntotal + nb, ntotal, stream); // (the two steps that can fail, before anything changes)
		if (coarse)
			dir.reserve(ntotal + nb);
		laps.lap("growth allocation + copy of the old rows", stream);
		stream_wait(stream, o.stream);
		launch_merge_append_rows(o.store.codes(), nullptr, nb, store.pitch, store.codes(), ntotal, stream);
		MVS_HIP(hipStreamSynchronize(stream));
		laps.lap("move kernel", stream);
		if (coarse)
			dir.append_from(o.dir, add_id);
		laps.lap("directory append", stream);
		ntotal += nb;
		lists_changed();
	}
	o.use_device();
	o.ntotal = 0;
	o.dir.assign.clear(), o.dir.ids.clear();
	o.store.release();
	o.lists_changed();
	use_device();
	laps.lap("the source's reset (its store is freed)", stream);
}
// IndexIVF::copy_subset_to: the predicate runs over the host directory, the selected code rows are gathered to the tail of other's store
void CodedListsIndex::copy_subset_to(IndexBase &other, int subset_type, int64_t a1, int64_t a2) {
	if (!coarse)
		return IndexBase::copy_subset_to(other, subset_type, a1, a2);
	check_compatible_for_merge(other);
	merge_check_subset_type(subset_type, a1);
	CodedListsIndex &o = static_cast<CodedListsIndex &>(other);
	const std::vector<int64_t> pos = dir.subset(subset_type, a1, a2, ntotal);
	const int64_t n = (int64_t)pos.size();
	if (n == 0)
		return;
	o.use_device();
	o.check_rows(o.ntotal + n);
	o.store.grow(o.ntotal + n, o.ntotal, o.stream);
	o.dir.reserve(o.ntotal + n);
	DevBuf dpos;
	dpos.reserve((size_t)n * sizeof(int64_t));
	MVS_HIP(hipMemcpyAsync(dpos.p, pos.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, o.stream));
	stream_wait(o.stream, stream);
	launch_merge_append_rows(store.codes(), (const int64_t *)dpos.p, n, store.pitch, o.store.codes(), o.ntotal, o.stream);
	MVS_HIP(hipStreamSynchronize(o.stream));
	o.dir.append_from(dir, 0, &pos);
	o.ntotal += n;
	o.lists_changed();
	use_device();
}

} // namespace mvs
