// compat/faiss_adaptor.cpp -- the faiss:: classes of compat/faiss/*.h implemented over the C ABI
// (include/mi355_faiss.h).  Built as libfaiss_mi355.so: the library the reference's CMake would link in place of
// `add_subdirectory(faiss)` / target `faiss` (/root/reference/CMakeLists.txt:58,67-71).
#include "faiss/Index.h"
#include "faiss/IndexBinary.h"
#include "faiss/IndexBinaryFlat.h"
#include "faiss/IndexFlat.h"
#include "faiss/IndexHNSW.h"
#include "faiss/IndexIDMap.h"
#include "faiss/IndexIVF.h"
#include "faiss/IndexPreTransform.h"
#include "faiss/IndexRefine.h"
#include "faiss/gpu/GpuCloner.h"
#include "faiss/gpu/GpuIndexIVF.h"
#include "faiss/index_factory.h"
#include "faiss/index_io.h"

#include <cstring>
#include <memory>

namespace faiss {

void throw_last_error() {
	throw FaissException(mvs_last_error());
}

void Index::refresh() {
	d = mvs_index_d(handle);
	ntotal = mvs_index_ntotal(handle);
	is_trained = mvs_index_is_trained(handle) != 0;
	metric_type = (MetricType)mvs_index_metric_type(handle);
}
Index::~Index() {
	if (handle && owns_handle)
		mvs_index_free(handle);
}
void Index::train(idx_t n, const float *x) {
	if (mvs_index_train(handle, n, x))
		throw_last_error();
	refresh();
}
void Index::add(idx_t n, const float *x) {
	before_add();
	if (mvs_index_add(handle, n, x)) {
		refresh();
		throw_last_error();
	}
	refresh();
}
void Index::add_with_ids(idx_t n, const float *x, const idx_t *xids) {
	before_add();
	if (mvs_index_add_with_ids(handle, n, x, xids)) {
		refresh();
		throw_last_error();
	}
	refresh();
}

// One IDSelector as the C ABI's triple.  IDSelectorBitmap / IDSelectorBatch, the two the glue builds, stay MVS_SEL_BITMAP / MVS_SEL_BATCH;
// a tree of the other classes is flattened to the postfix nodes of one MVS_SEL_PROGRAM (include/mi355_faiss.h "selector programs").  The
// nodes live in a buffer of the calling thread until its next call here: long enough for the C ABI call that follows.  A class that is
// none of these throws `unknown`
static bool flatten_selector(const IDSelector *sel, std::vector<mvs_sel_node> &nodes) {
	mvs_sel_node nd;
	memset(&nd, 0, sizeof nd);
	if (!sel)
		return false;
	if (auto bm = dynamic_cast<const IDSelectorBitmap *>(sel)) {
		nd.op = MVS_SELOP_BITMAP, nd.data = bm->bitmap, nd.n = (int64_t)bm->n;
	} else if (auto bt = dynamic_cast<const IDSelectorBatch *>(sel)) {
		nd.op = MVS_SELOP_BATCH, nd.data = bt->ids.data(), nd.n = (int64_t)bt->ids.size();
	} else if (auto ar = dynamic_cast<const IDSelectorArray *>(sel)) {
		nd.op = MVS_SELOP_ARRAY, nd.data = ar->ids, nd.n = (int64_t)ar->n;
	} else if (auto rg = dynamic_cast<const IDSelectorRange *>(sel)) {
		nd.op = MVS_SELOP_RANGE, nd.imin = rg->imin, nd.imax = rg->imax;
	} else if (dynamic_cast<const IDSelectorAll *>(sel)) {
		nd.op = MVS_SELOP_ALL;
	} else if (auto nt = dynamic_cast<const IDSelectorNot *>(sel)) {
		if (!flatten_selector(nt->sel, nodes))
			return false;
		nd.op = MVS_SELOP_NOT;
	} else {
		const IDSelector *lhs = nullptr, *rhs = nullptr;
		if (auto a = dynamic_cast<const IDSelectorAnd *>(sel))
			nd.op = MVS_SELOP_AND, lhs = a->lhs, rhs = a->rhs;
		else if (auto o = dynamic_cast<const IDSelectorOr *>(sel))
			nd.op = MVS_SELOP_OR, lhs = o->lhs, rhs = o->rhs;
		else if (auto x = dynamic_cast<const IDSelectorXOr *>(sel))
			nd.op = MVS_SELOP_XOR, lhs = x->lhs, rhs = x->rhs;
		else
			return false;
		if (!flatten_selector(lhs, nodes) || !flatten_selector(rhs, nodes))
			return false;
	}
	nodes.push_back(nd);
	return true;
}
static void selector_triple(const IDSelector *sel, const char *unknown, int32_t *kind, const void **data, int64_t *n) {
	if (auto bm = dynamic_cast<const IDSelectorBitmap *>(sel)) {
		*kind = MVS_SEL_BITMAP, *data = bm->bitmap, *n = (int64_t)bm->n;
		return;
	}
	if (auto bt = dynamic_cast<const IDSelectorBatch *>(sel)) {
		*kind = MVS_SEL_BATCH, *data = bt->ids.data(), *n = (int64_t)bt->ids.size();
		return;
	}
	static thread_local std::vector<mvs_sel_node> nodes;
	nodes.clear();
	if (!flatten_selector(sel, nodes))
		throw FaissException(unknown);
	*kind = MVS_SEL_PROGRAM, *data = nodes.data(), *n = (int64_t)nodes.size(); // (more than 64 nodes: the library says so)
}

// innerCreateSearchParameters (src/faiss_extension.cpp:668-721) hands us SearchParameters / SearchParametersIVF /
// SearchParametersHNSW with an optional IDSelectorBitmap / IDSelectorBatch
void fill_params(const Index *, const SearchParameters *params, mvs_search_params *out) {
	memset(out, 0, sizeof *out);
	if (!params)
		return;
	if (auto ivf = dynamic_cast<const SearchParametersIVF *>(params)) {
		out->nprobe = (int64_t)ivf->nprobe;
		// IVF<n>_HNSW<m>: the glue hangs the coarse quantizer's SearchParametersHNSW here (:679-681)
		if (auto qh = dynamic_cast<const SearchParametersHNSW *>(ivf->quantizer_params))
			out->efSearch = qh->efSearch;
	}
	if (auto hnsw = dynamic_cast<const SearchParametersHNSW *>(params))
		out->efSearch = hnsw->efSearch;
	if (params->sel)
		selector_triple(params->sel, "Error in faiss::Index::search: this IDSelector type is not implemented on the MI355X path", &out->sel_kind,
		                &out->sel_data, &out->sel_n);
}
void Index::search(idx_t n, const float *x, idx_t k, float *distances, idx_t *labels,
                   const SearchParameters *params) const {
	mvs_search_params p;
	fill_params(this, params, &p);
	before_search();
	if (mvs_index_search(handle, n, x, k, distances, labels, &p))
		throw_last_error();
}

void Index::range_search(idx_t n, const float *x, float radius, RangeSearchResult *result, const SearchParameters *params) const {
	mvs_search_params p;
	fill_params(this, params, &p);
	before_search();
	mvs_range_result *raw = nullptr;
	if (mvs_index_range_search(handle, n, x, radius, &p, &raw))
		throw_last_error();
	std::unique_ptr<mvs_range_result, void (*)(mvs_range_result *)> r(raw, mvs_range_result_free); // (freed whatever throws below)
	const size_t nq = (size_t)mvs_range_result_nq(r.get());
	if (nq != result->nq) // (the caller sized lims for another batch)
		throw FaissException("Error in faiss::Index::range_search: result->nq differs from n");
	if (!result->lims)
		result->lims = new size_t[nq + 1];
	const int64_t *lims = mvs_range_result_lims(r.get());
	for (size_t q = 0; q <= nq; ++q)
		result->lims[q] = (size_t)lims[q];
	result->do_allocation();
	const size_t total = result->lims[nq];
	if (total > 0) {
		memcpy(result->distances, mvs_range_result_distances(r.get()), total * sizeof(float));
		memcpy(result->labels, mvs_range_result_labels(r.get()), total * sizeof(idx_t));
	}
}

// the selector classes fill_params translates; any other class throws
size_t Index::remove_ids(const IDSelector &sel) {
	int32_t kind = MVS_SEL_NONE;
	const void *data = nullptr;
	int64_t n = 0;
	selector_triple(&sel, "Error in faiss::Index::remove_ids: this IDSelector type is not implemented on the MI355X path", &kind, &data, &n);
	int64_t removed = 0;
	const int rc = mvs_index_remove_ids(handle, kind, data, n, &removed);
	refresh_chain();
	if (rc)
		throw_last_error();
	return (size_t)removed;
}

// include/mi355_faiss.h "merge_from and copy_subset_to": both wrappers read their counts again whatever the outcome
void Index::merge_from(Index &otherIndex, idx_t add_id) {
	const int rc = mvs_index_merge_from(handle, otherIndex.handle, add_id);
	refresh_chain();
	otherIndex.refresh_chain();
	if (rc)
		throw_last_error();
}
void Index::check_compatible_for_merge(const Index &otherIndex) const {
	if (mvs_index_check_compatible_for_merge(handle, otherIndex.handle))
		throw_last_error();
}
void IndexIVF::copy_subset_to(IndexIVF &other, InvertedLists::subset_type_t subset_type, idx_t a1, idx_t a2) const {
	const int rc = mvs_index_ivf_copy_subset_to(handle, other.handle, (int)subset_type, a1, a2);
	other.refresh_chain();
	if (rc)
		throw_last_error();
}

void Index::reconstruct(idx_t key, float *recons) const {
	if (mvs_index_reconstruct(handle, key, recons))
		throw_last_error();
}
void Index::reconstruct_batch(idx_t n, const idx_t *keys, float *recons) const {
	if (mvs_index_reconstruct_batch(handle, n, keys, recons))
		throw_last_error();
}
void Index::reconstruct_n(idx_t i0, idx_t ni, float *recons) const {
	if (mvs_index_reconstruct_n(handle, i0, ni, recons))
		throw_last_error();
}
void Index::search_and_reconstruct(idx_t n, const float *x, idx_t k, float *distances, idx_t *labels, float *recons,
                                   const SearchParameters *params) const {
	mvs_search_params p;
	fill_params(this, params, &p);
	before_search();
	if (mvs_index_search_and_reconstruct(handle, n, x, k, distances, labels, recons, &p))
		throw_last_error();
}

void IndexIDMap::refresh_chain() {
	refresh();
	if (index)
		index->refresh_chain();
}
IndexIDMap::~IndexIDMap() {
	delete index;
}
void IndexIDMap::before_add() {
	if (index)
		index->before_add();
}
void IndexIDMap::before_search() const {
	if (index)
		index->before_search();
}
IndexRefine::~IndexRefine() {
	delete base_index;
	delete refine_index;
}
void IndexRefine::before_search() const {
	if (mvs_index_refine_set_k_factor(handle, k_factor))
		throw_last_error();
}
void VectorTransform::refresh() {
	int type = 0, hb = 0, tr = 0;
	if (mvs_index_pretransform_info(handle, slot, &type, &d_in, &d_out, &hb, &tr))
		throw_last_error();
	is_trained = tr != 0;
	if (auto *lt = dynamic_cast<LinearTransform *>(this))
		lt->have_bias = hb != 0;
}
std::vector<float> LinearTransform::get_A() const {
	std::vector<float> A((size_t)d_in * d_out);
	if (mvs_index_pretransform_get_linear(handle, slot, A.data(), nullptr))
		throw_last_error();
	return A;
}
std::vector<float> LinearTransform::get_b() const {
	std::vector<float> b((size_t)d_out);
	if (mvs_index_pretransform_get_linear(handle, slot, nullptr, b.data()))
		throw_last_error();
	return b;
}
std::vector<float> PCAMatrix::get_mean() const {
	std::vector<float> m((size_t)d_in);
	if (mvs_index_pretransform_get_pca(handle, slot, m.data(), nullptr))
		throw_last_error();
	return m;
}
std::vector<float> PCAMatrix::get_eigenvalues() const {
	std::vector<float> e((size_t)d_in);
	if (mvs_index_pretransform_get_pca(handle, slot, nullptr, e.data()))
		throw_last_error();
	return e;
}
IndexPreTransform::~IndexPreTransform() {
	for (VectorTransform *t : chain)
		delete t;
	delete index;
}
void IndexPreTransform::refresh_chain() {
	refresh();
	for (VectorTransform *t : chain)
		t->refresh();
	if (index)
		index->refresh_chain();
}
void IndexPreTransform::before_add() {
	if (index)
		index->before_add();
}
void IndexPreTransform::before_search() const {
	if (index)
		index->before_search();
}
const float *IndexPreTransform::apply_chain(idx_t n, const float *x) const {
	const int dout = chain.empty() ? d : chain.back()->d_out;
	float *out = new float[(size_t)n * dout];
	if (mvs_index_pretransform_apply(handle, n, x, out)) {
		delete[] out;
		throw_last_error();
	}
	return out;
}
IndexIVF::~IndexIVF() {
	delete quantizer;
}
IndexHNSWSQ::~IndexHNSWSQ() {
	delete storage;
}
void IndexHNSW::before_add() {
	(void)mvs_index_hnsw_set_ef_construction(handle, hnsw.efConstruction);
}

Index *Index::wrap(mvs_index *h, bool owned) {
	Index *ix = nullptr;
	switch (mvs_index_kind(h)) {
	case MVS_KIND_IDMAP: {
		auto *m = new IndexIDMap;
		m->handle = h;
		m->index = wrap(mvs_index_idmap_sub(h), false);
		ix = m;
		break;
	}
	case MVS_KIND_IVFFLAT: {
		auto *v = new IndexIVFFlat;
		v->handle = h;
		if (mvs_index *q = mvs_index_ivf_quantizer(h)) {
			v->quantizer = wrap(q, false);
			v->nlist = (size_t)mvs_index_ntotal(q);
		}
		ix = v;
		break;
	}
	case MVS_KIND_IVFPQ: {
		auto *v = new IndexIVFPQ;
		v->handle = h;
		if (mvs_index *q = mvs_index_ivf_quantizer(h))
			v->quantizer = wrap(q, false);
		v->nlist = (size_t)mvs_index_ivf_nlist(h); // (the quantizer is empty until the index is trained)
		int M = 0, nbits = 0;
		if (mvs_index_pq_info(h, &M, &nbits))
			throw_last_error();
		v->pq.d = (size_t)mvs_index_d(h);
		v->pq.M = (size_t)M;
		v->pq.nbits = (size_t)nbits;
		v->pq.dsub = v->pq.d / v->pq.M;
		v->pq.ksub = (size_t)1 << nbits;
		v->pq.code_size = v->pq.M;
		ix = v;
		break;
	}
	case MVS_KIND_IVFSQ: {
		auto *v = new IndexIVFScalarQuantizer;
		v->handle = h;
		if (mvs_index *q = mvs_index_ivf_quantizer(h))
			v->quantizer = wrap(q, false);
		v->nlist = (size_t)mvs_index_ivf_nlist(h); // (the quantizer is empty until the index is trained)
		v->sq.d = v->sq.code_size = (size_t)mvs_index_d(h);
		ix = v;
		break;
	}
	case MVS_KIND_SQ: {
		auto *s = new IndexScalarQuantizer;
		s->handle = h;
		s->sq.d = s->sq.code_size = (size_t)mvs_index_d(h);
		ix = s;
		break;
	}
	case MVS_KIND_REFINE: {
		auto *r = new IndexRefineFlat;
		r->handle = h;
		r->base_index = wrap(mvs_index_refine_base(h), false);
		r->refine_index = wrap(mvs_index_refine_store(h), false);
		if (mvs_index_refine_get_k_factor(h, &r->k_factor))
			throw_last_error();
		ix = r;
		break;
	}
	case MVS_KIND_PRETRANSFORM: {
		auto *p = new IndexPreTransform;
		p->handle = h;
		p->index = wrap(mvs_index_pretransform_sub(h), false);
		for (int i = 0; i < mvs_index_pretransform_count(h); ++i) {
			int type = 0;
			if (mvs_index_pretransform_info(h, i, &type, nullptr, nullptr, nullptr, nullptr))
				throw_last_error();
			VectorTransform *t = type == MVS_VT_NORM ? (VectorTransform *)new NormalizationTransform
			                                         : (type == MVS_VT_PCA ? (VectorTransform *)new PCAMatrix : (VectorTransform *)new LinearTransform);
			t->handle = h, t->slot = i;
			t->refresh();
			p->chain.push_back(t);
		}
		ix = p;
		break;
	}
	case MVS_KIND_HNSW:
		ix = new IndexHNSWFlat;
		ix->handle = h;
		break;
	case MVS_KIND_HNSWSQ: {
		auto *w = new IndexHNSWSQ;
		w->handle = h;
		auto *s = new IndexScalarQuantizer; // a view: the codes live in the device index
		s->handle = h;
		s->owns_handle = false;
		s->sq.d = s->sq.code_size = (size_t)mvs_index_d(h);
		s->refresh();
		w->storage = s;
		ix = w;
		break;
	}
	case MVS_KIND_PQ: {
		auto *p = new IndexPQ;
		p->handle = h;
		int M = 0, nbits = 0;
		if (mvs_index_pq_info(h, &M, &nbits))
			throw_last_error();
		p->pq.d = (size_t)mvs_index_d(h);
		p->pq.M = (size_t)M;
		p->pq.nbits = (size_t)nbits;
		p->pq.dsub = p->pq.d / p->pq.M;
		p->pq.ksub = (size_t)1 << nbits;
		p->pq.code_size = p->pq.M;
		ix = p;
		break;
	}
	default:
		if (mvs_index_metric_type(h) == METRIC_L2)
			ix = new IndexFlatL2;
		else if (mvs_index_metric_type(h) == METRIC_INNER_PRODUCT)
			ix = new IndexFlatIP;
		else
			ix = new IndexFlat;
		ix->handle = h;
	}
	ix->owns_handle = owned;
	ix->refresh();
	return ix;
}

Index *index_factory(int d, const char *description, MetricType metric) {
	mvs_index *h = nullptr;
	if (mvs_index_factory(&h, d, description, (int)metric))
		throw_last_error();
	return Index::wrap(h, true);
}
void write_index(const Index *idx, const char *fname) {
	if (mvs_write_index(idx->handle, fname))
		throw_last_error();
}
Index *read_index(const char *fname, int) {
	mvs_index *h = nullptr;
	if (mvs_read_index(&h, fname))
		throw_last_error();
	return Index::wrap(h, true);
}

// ---- faiss::IndexBinary and its kin over mvs_binary_index (include/mi355_faiss.h "binary indexes")
void IndexBinary::refresh() {
	d = mvs_binary_index_d(handle);
	code_size = mvs_binary_index_code_size(handle);
	ntotal = mvs_binary_index_ntotal(handle);
}
IndexBinary::~IndexBinary() {
	if (handle && owns_handle)
		mvs_binary_index_free(handle);
}
void IndexBinary::train(idx_t, const uint8_t *) {
}
void IndexBinary::add(idx_t n, const uint8_t *x) {
	const int rc = mvs_binary_index_add(handle, n, x);
	refresh();
	if (rc)
		throw_last_error();
}
void IndexBinary::add_with_ids(idx_t n, const uint8_t *x, const idx_t *xids) {
	const int rc = mvs_binary_index_add_with_ids(handle, n, x, xids);
	refresh();
	if (rc)
		throw_last_error();
}
void IndexBinary::search(idx_t n, const uint8_t *x, idx_t k, int32_t *distances, idx_t *labels, const SearchParameters *params) const {
	mvs_search_params p;
	fill_params(nullptr, params, &p);
	if (mvs_binary_index_search(handle, n, x, k, distances, labels, &p))
		throw_last_error();
}
void IndexBinary::range_search(idx_t n, const uint8_t *x, int radius, RangeSearchResult *result, const SearchParameters *params) const {
	mvs_search_params p;
	fill_params(nullptr, params, &p);
	mvs_range_result *raw = nullptr;
	if (mvs_binary_index_range_search(handle, n, x, radius, &p, &raw))
		throw_last_error();
	std::unique_ptr<mvs_range_result, void (*)(mvs_range_result *)> r(raw, mvs_range_result_free);
	const size_t nq = (size_t)mvs_range_result_nq(r.get());
	if (nq != result->nq)
		throw FaissException("Error in faiss::IndexBinary::range_search: result->nq differs from n");
	if (!result->lims)
		result->lims = new size_t[nq + 1];
	const int64_t *lims = mvs_range_result_lims(r.get());
	for (size_t q = 0; q <= nq; ++q)
		result->lims[q] = (size_t)lims[q];
	result->do_allocation();
	const size_t total = result->lims[nq];
	if (total > 0) {
		memcpy(result->distances, mvs_range_result_distances(r.get()), total * sizeof(float));
		memcpy(result->labels, mvs_range_result_labels(r.get()), total * sizeof(idx_t));
	}
}
void IndexBinary::reset() {
	const int rc = mvs_binary_index_reset(handle);
	refresh();
	if (rc)
		throw_last_error();
}
void IndexBinary::reconstruct(idx_t key, uint8_t *recons) const {
	if (mvs_binary_index_reconstruct(handle, key, recons))
		throw_last_error();
}
void IndexBinary::reconstruct_n(idx_t i0, idx_t ni, uint8_t *recons) const {
	if (mvs_binary_index_reconstruct_n(handle, i0, ni, recons))
		throw_last_error();
}
size_t IndexBinary::remove_ids(const IDSelector &) {
	throw FaissException("Error in virtual size_t faiss::IndexBinary::remove_ids(const faiss::IDSelector&) at faiss/IndexBinary.cpp: "
	                     "remove_ids not implemented for this type of index");
}
void IndexBinary::merge_from(IndexBinary &, idx_t) {
	throw FaissException("Error in virtual void faiss::IndexBinary::merge_from(faiss::IndexBinary&, faiss::idx_t) at faiss/IndexBinary.cpp: "
	                     "merge_from() not implemented");
}
void IndexBinary::check_compatible_for_merge(const IndexBinary &) const {
	throw FaissException("Error in virtual void faiss::IndexBinary::check_compatible_for_merge(const faiss::IndexBinary&) const at faiss/IndexBinary.cpp: "
	                     "check_compatible_for_merge() not implemented");
}
IndexBinaryFlat::IndexBinaryFlat(idx_t d_) {
	if (mvs_binary_index_factory(&handle, (int)d_, "BFlat"))
		throw_last_error();
	refresh();
}
// the wrapped index must be empty: its rows live in the device object the wrapper creates, and `index` becomes a view of that object's
// own IndexBinaryFlat.  The object handed in is left alone (and deleted with the wrapper if own_fields is set)
IndexBinaryIDMap::IndexBinaryIDMap(IndexBinary *wrapped) {
	if (!wrapped || wrapped->ntotal != 0)
		throw FaissException("Error in faiss::IndexBinaryIDMap::IndexBinaryIDMap(faiss::IndexBinary*): index must be empty on input");
	if (mvs_binary_index_factory(&handle, wrapped->d, "IDMap,BFlat"))
		throw_last_error();
	given_ = wrapped;
	IndexBinaryIDMap::refresh();
}
IndexBinaryIDMap::~IndexBinaryIDMap() {
	delete index; // (a view: its handle is borrowed)
	if (own_fields)
		delete given_;
}
void IndexBinaryIDMap::refresh() {
	IndexBinary::refresh();
	if (!index) {
		if (mvs_binary_index *sub = mvs_binary_index_idmap_sub(handle)) {
			index = new IndexBinaryFlat;
			index->handle = sub;
			index->owns_handle = false;
		}
	}
	if (index)
		index->refresh();
}
IndexBinary *IndexBinary::wrap(mvs_binary_index *h, bool owned) {
	IndexBinary *ix = mvs_binary_index_kind(h) == MVS_BINARY_KIND_IDMAP ? (IndexBinary *)new IndexBinaryIDMap : (IndexBinary *)new IndexBinaryFlat;
	ix->handle = h;
	ix->owns_handle = owned;
	ix->refresh();
	return ix;
}
IndexBinary *index_binary_factory(int d, const char *description) {
	mvs_binary_index *h = nullptr;
	if (mvs_binary_index_factory(&h, d, description))
		throw_last_error();
	return IndexBinary::wrap(h, true);
}
void write_index_binary(const IndexBinary *idx, const char *fname) {
	if (mvs_write_index_binary(idx->handle, fname))
		throw_last_error();
}
IndexBinary *read_index_binary(const char *fname, int) {
	mvs_binary_index *h = nullptr;
	if (mvs_read_index_binary(&h, fname))
		throw_last_error();
	return IndexBinary::wrap(h, true);
}

namespace gpu {
faiss::Index *index_cpu_to_gpu(GpuResourcesProvider *, int device, const faiss::Index *index) {
	mvs_index *h = nullptr;
	if (mvs_index_clone_to_gpu(&h, index->handle, device))
		throw_last_error();
	return Index::wrap(h, true);
}
} // namespace gpu

} // namespace faiss
