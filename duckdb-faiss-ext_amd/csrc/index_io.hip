// csrc/index_io.hip -- faiss::write_index / faiss::read_index (src/faiss_extension.cpp:199,234).
//
// FAISS's on-disk format [UPSTREAM: faiss/impl/index_write.cpp, index_read.cpp, impl/io_macros.h], restated:
//   little-endian; every index starts with a 4-byte fourcc (c0 | c1<<8 | c2<<16 | c3<<24) and the common header
//     int d; idx_t ntotal; idx_t dummy = 1<<20 (x2); bool is_trained (1 byte); int metric_type; [float metric_arg
//     only when metric_type > 1]
//   vectors are "size_t n" followed by n elements.
//   IxFI / IxF2 / IxFl  IndexFlatIP / IndexFlatL2 / IndexFlat : header, size_t nfloat, nfloat * f32
//   IxMp / IxM2         IndexIDMap / IndexIDMap2              : header, sub-index, vector<idx_t> id_map
//   IwFl                IndexIVFFlat : ivf header = {header, size_t nlist, size_t nprobe, quantizer index, direct map
//                       (char type, vector<idx_t> array [, hashtable pairs])}, then the inverted lists:
//                       "ilar", size_t nlist, size_t code_size, list sizes ("full": vector<size_t> of nlist sizes, or
//                       "sprs": vector<size_t> of (list_no, size) pairs), then per non-empty list codes, then ids
//   IHNf                IndexHNSWFlat : header, struct HNSW {vector<double> assign_probas, vector<int>
//                       cum_nneighbor_per_level, vector<int> levels, vector<size_t> offsets, vector<int32> neighbors,
//                       int32 entry_point, int max_level, int efConstruction, int efSearch, int upper_beam(=1)},
//                       then the storage index
//   IHNs                IndexHNSWSQ : the header and struct HNSW exactly as IHNf writes them, then the storage as an IxSQ image.  IHNs over a
//                       Flat storage and IHNf over an IxSQ storage are refused on reading
//   IwPQ                IndexIVFPQ : the ivf header exactly as IwFl writes it, uint8 by_residual (1), size_t code_size (= M),
//                       ProductQuantizer {size_t d, M, nbits; vector<float> centroids}, then the inverted lists ("ilar", code_size = M:
//                       per list M-byte codes, then ids).  by_residual = 0, nbits != 8 and IwQR (IndexIVFPQR) are refused on reading
//   IxPq                IndexPQ : header, ProductQuantizer {size_t d, M, nbits; vector<float> centroids [M][ksub][dsub]}, vector<uint8_t>
//                       codes [ntotal][M], int32 search_type (0 = ST_PQ), uint8 encode_signs, int32 polysemous_ht
//   IxSQ                IndexScalarQuantizer : header, ScalarQuantizer {int qtype (0 = QT_8bit), int rangestat (0), float rangestat_arg (0),
//                       size_t d, size_t code_size (= d), vector<float> trained = vmin [d] | vdiff [d]}, vector<uint8_t> codes [ntotal][d]
//   IwSq                IndexIVFScalarQuantizer : the ivf header exactly as IwFl writes it, the ScalarQuantizer block, size_t code_size (= d),
//                       uint8 by_residual (1), then the inverted lists ("ilar", code_size = d).  Another qtype, by_residual = 0 and
//                       code_size != d are refused on reading
//   IxRF                IndexRefine / IndexRefineFlat : header, the base index, the refine index (here always IxF2 / IxFI), float k_factor.
//                       Any other second index, and sub-indexes that disagree in d, metric or ntotal, are refused on reading
//   IxPT                IndexPreTransform : header (d = the chain's input dimension), int32 n, n vector transforms, then the sub-index.  One
//                       transform = its fourcc; for "PcAm" (PCAMatrix) float eigen_power, float epsilon (the old "PCAm" lacks epsilon),
//                       uint8 random_rotation, int32 balanced_bins, vector<float> mean, eigenvalues, PCAMat; for every linear kind ("LTra",
//                       "rrot", "PCAm", "PcAm") uint8 have_bias, vector<float> A [d_out][d_in], vector<float> b; for "VNrm" float norm; for all
//                       int32 d_in, int32 d_out, uint8 is_trained.  Written: PCA / PCAW as "PcAm", L2norm as "VNrm", a set or loaded plain matrix
//                       as "LTra".  Read: "LTra", "rrot", "PCAm", "PcAm" as linear transforms, "VNrm" with norm 2; every other transform
//                       ("RmDT", "VCnt", "Viqt", "Viqm", "opqm", ...) is refused by name, as are sizes and dimensions that do not fit
//                       (csrc/pretransform.hip check_chain).  RESTATED FROM MEMORY like the rest: no FAISS source was at hand
// No .index file written by FAISS itself exists in the reference or in this image, so byte compatibility is
// "restated, unverified against a real file" (DESIGN.md); the round trip through this reader is tested.
#include "index.h"

#include <cerrno>
#include <cstring>

namespace mvs {

namespace {

constexpr uint32_t fourcc(const char (&s)[5]) {
	return (uint32_t)(unsigned char)s[0] | ((uint32_t)(unsigned char)s[1] << 8) | ((uint32_t)(unsigned char)s[2] << 16) |
	       ((uint32_t)(unsigned char)s[3] << 24);
}

struct Writer {
	FILE *f;
	const char *name;
	void raw(const void *p, size_t n) {
		if (n && fwrite(p, 1, n, f) != n)
			throw_faiss("void faiss::write_index(const faiss::Index*, const char*)", "faiss/impl/index_write.cpp",
			            "write error in %s: %s", name, strerror(errno));
	}
	template <typename T>
	void one(const T &v) {
		raw(&v, sizeof(T));
	}
	template <typename T>
	void vec(const std::vector<T> &v) {
		const uint64_t n = v.size();
		one(n);
		raw(v.data(), n * sizeof(T));
	}
};

struct Reader {
	FILE *f;
	const char *name;
	void raw(void *p, size_t n) {
		if (n && fread(p, 1, n, f) != n)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "read error in %s: %s", name, feof(f) ? "unexpected end of file" : strerror(errno));
	}
	template <typename T>
	void one(T &v) {
		raw(&v, sizeof(T));
	}
	template <typename T>
	void vec(std::vector<T> &v) {
		uint64_t n = 0;
		one(n);
		if (n > ((uint64_t)1 << 40) / sizeof(T))
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "Error: 'size >= 0 && size < (uint64_t{1} << 40)' failed in %s", name);
		v.resize((size_t)n);
		raw(v.data(), (size_t)n * sizeof(T));
	}
};

void write_header(Writer &w, const HostIndex &h) {
	const int32_t d = h.d;
	const int64_t ntotal = h.ntotal, dummy = 1 << 20;
	const uint8_t trained = h.is_trained ? 1 : 0;
	const int32_t metric = h.metric;
	w.one(d);
	w.one(ntotal);
	w.one(dummy);
	w.one(dummy);
	w.one(trained);
	w.one(metric);
	if (metric > 1) {
		const float metric_arg = h.metric_arg;
		w.one(metric_arg);
	}
}
void read_header(Reader &r, HostIndex &h) {
	int32_t d = 0, metric = 0;
	int64_t ntotal = 0, dummy = 0;
	uint8_t trained = 0;
	r.one(d);
	r.one(ntotal);
	r.one(dummy);
	r.one(dummy);
	r.one(trained);
	r.one(metric);
	if (metric > 1) {
		float metric_arg;
		r.one(metric_arg);
		h.metric_arg = metric_arg;
	}
	h.d = d;
	h.ntotal = ntotal;
	h.is_trained = trained != 0;
	h.metric = metric;
}

void write_image(Writer &w, const HostIndex &h);
// write_ivf_header: header, nlist, nprobe, the quantizer, the direct map (DirectMap::NoMap)
void write_ivf_header(Writer &w, const HostIndex &h) {
	write_header(w, h);
	const uint64_t nlist = (uint64_t)h.nlist, nprobe = (uint64_t)h.nprobe;
	w.one(nlist);
	w.one(nprobe);
	write_image(w, *h.sub);
	const char direct_map_type = 0;
	w.one(direct_map_type);
	w.vec(std::vector<int64_t>());
}
// write_InvertedLists (ArrayInvertedLists): per non-empty list its codes (code_size bytes a row), then its ids
template <typename T>
void write_lists(Writer &w, uint64_t nlist, uint64_t code_size, const std::vector<std::vector<int64_t>> &ids, const std::vector<std::vector<T>> &codes) {
	w.one(fourcc("ilar"));
	w.one(nlist);
	w.one(code_size);
	uint64_t n_non0 = 0;
	for (const auto &l : ids)
		n_non0 += l.empty() ? 0 : 1;
	std::vector<uint64_t> sizes;
	if (n_non0 > nlist / 2) {
		w.one(fourcc("full"));
		for (const auto &l : ids)
			sizes.push_back(l.size());
	} else {
		w.one(fourcc("sprs"));
		for (size_t i = 0; i < ids.size(); i++)
			if (!ids[i].empty()) {
				sizes.push_back(i);
				sizes.push_back(ids[i].size());
			}
	}
	w.vec(sizes);
	for (size_t i = 0; i < ids.size(); i++)
		if (!ids[i].empty()) {
			w.raw(codes[i].data(), codes[i].size() * sizeof(T));
			w.raw(ids[i].data(), ids[i].size() * sizeof(int64_t));
		}
}

// write_ScalarQuantizer / read_ScalarQuantizer: QT_8bit with RS_minmax only
void write_sq_block(Writer &w, const HostIndex &h) {
	const int32_t qtype = 0, rangestat = 0;
	const float rangestat_arg = 0.f;
	const uint64_t d = (uint64_t)h.d, code_size = (uint64_t)h.d;
	w.one(qtype);
	w.one(rangestat);
	w.one(rangestat_arg);
	w.one(d);
	w.one(code_size);
	w.vec(h.sq_has_range ? h.sq_trained : std::vector<float>()); // (FAISS fills `trained` at training: an untrained quantizer stores none)
}
void read_sq_block(Reader &r, HostIndex &h, const char *kind) {
	int32_t qtype = 0, rangestat = 0;
	float rangestat_arg = 0.f;
	uint64_t d = 0, code_size = 0;
	r.one(qtype);
	r.one(rangestat);
	r.one(rangestat_arg);
	r.one(d);
	r.one(code_size);
	if (qtype != 0)
		throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
		            "%s with ScalarQuantizer qtype = %d is not implemented on the MI355X path (QT_8bit only)", kind, qtype);
	if (d != (uint64_t)h.d || code_size != d)
		throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
		            "%s with d = %llu, code_size = %llu is not implemented on the MI355X path (one byte per component only)", kind,
		            (unsigned long long)d, (unsigned long long)code_size);
	r.vec(h.sq_trained);
	if (h.sq_trained.size() != 2 * (size_t)d) {
		if (!h.sq_trained.empty())
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "%s: %zu trained values for d = %llu", kind, h.sq_trained.size(), (unsigned long long)d);
		h.sq_trained.assign(2 * (size_t)d, 0.f); // (an untrained quantizer stores none)
	} else {
		h.sq_has_range = true;
	}
}

void write_image(Writer &w, const HostIndex &h) {
	switch (h.kind) {
	case MVS_KIND_FLAT: {
		w.one(h.metric == METRIC_IP ? fourcc("IxFI") : (h.metric == METRIC_L2 ? fourcc("IxF2") : fourcc("IxFl")));
		write_header(w, h);
		w.vec(h.rows); // WRITEXBVECTOR: count of floats, then the codes
		return;
	}
	case MVS_KIND_IDMAP: {
		w.one(h.idmap2 ? fourcc("IxM2") : fourcc("IxMp"));
		write_header(w, h);
		write_image(w, *h.sub);
		w.vec(h.ids);
		return;
	}
	case MVS_KIND_IVFFLAT: {
		w.one(fourcc("IwFl"));
		write_ivf_header(w, h);
		const uint64_t nlist = (uint64_t)h.nlist;
		write_lists(w, nlist, (uint64_t)h.d * sizeof(float), h.list_ids, h.list_codes);
		return;
	}
	case MVS_KIND_IVFPQ: {
		w.one(fourcc("IwPQ"));
		write_ivf_header(w, h);
		const uint8_t by_residual = 1;
		const uint64_t code_size = (uint64_t)h.pq_M, d = (uint64_t)h.d, M = (uint64_t)h.pq_M, nbits = 8;
		w.one(by_residual);
		w.one(code_size);
		w.one(d);
		w.one(M);
		w.one(nbits);
		w.vec(h.pq_centroids);
		write_lists(w, (uint64_t)h.nlist, code_size, h.list_ids, h.list_bytes);
		return;
	}
	case MVS_KIND_SQ: {
		w.one(fourcc("IxSQ"));
		write_header(w, h);
		write_sq_block(w, h);
		w.vec(h.sq_codes);
		return;
	}
	case MVS_KIND_IVFSQ: {
		w.one(fourcc("IwSq"));
		write_ivf_header(w, h);
		write_sq_block(w, h);
		const uint64_t code_size = (uint64_t)h.d;
		const uint8_t by_residual = 1;
		w.one(code_size);
		w.one(by_residual);
		write_lists(w, (uint64_t)h.nlist, code_size, h.list_ids, h.list_bytes);
		return;
	}
	case MVS_KIND_HNSW:
	case MVS_KIND_HNSWSQ: { // IHNs: the same header and HNSW block, then the storage as an IxSQ image
		w.one(h.kind == MVS_KIND_HNSWSQ ? fourcc("IHNs") : fourcc("IHNf"));
		write_header(w, h);
		w.vec(h.assign_probas);
		w.vec(h.cum_nneighbor_per_level);
		w.vec(h.levels);
		w.vec(h.offsets);
		w.vec(h.neighbors);
		w.one(h.entry_point);
		const int32_t ml = h.max_level, efc = h.efConstruction, efs = h.efSearch, upper_beam = 1;
		w.one(ml);
		w.one(efc);
		w.one(efs);
		w.one(upper_beam);
		write_image(w, *h.sub);
		return;
	}
	case MVS_KIND_REFINE: {
		w.one(fourcc("IxRF"));
		write_header(w, h);
		write_image(w, *h.sub);
		write_image(w, *h.sub2);
		w.one(h.k_factor);
		return;
	}
	case MVS_KIND_PRETRANSFORM: {
		w.one(fourcc("IxPT"));
		write_header(w, h);
		const int32_t nt = (int32_t)h.chain.size();
		w.one(nt);
		for (const HostTransform &t : h.chain) {
			if (t.type == MVS_VT_NORM) {
				w.one(fourcc("VNrm"));
				w.one(t.norm);
			} else {
				if (t.type == MVS_VT_PCA) {
					w.one(fourcc("PcAm"));
					w.one(t.eigen_power);
					w.one(t.epsilon);
					const uint8_t rr = t.random_rotation ? 1 : 0;
					w.one(rr);
					w.one(t.balanced_bins);
					w.vec(t.mean);
					w.vec(t.eigenvalues);
					w.vec(t.PCAMat);
				} else {
					w.one(fourcc("LTra"));
				}
				const uint8_t hb = t.have_bias ? 1 : 0;
				w.one(hb);
				w.vec(t.A);
				w.vec(t.b);
			}
			const int32_t di = t.d_in, dout = t.d_out;
			const uint8_t tr = t.is_trained ? 1 : 0;
			w.one(di);
			w.one(dout);
			w.one(tr);
		}
		write_image(w, *h.sub);
		return;
	}
	case MVS_KIND_PQ: {
		w.one(fourcc("IxPq"));
		write_header(w, h);
		const uint64_t d = (uint64_t)h.d, M = (uint64_t)h.pq_M, nbits = 8;
		w.one(d);
		w.one(M);
		w.one(nbits);
		w.vec(h.pq_centroids);
		w.vec(h.pq_codes);
		const int32_t search_type = 0, polysemous_ht = 8 * h.pq_M + 1;
		const uint8_t encode_signs = 0;
		w.one(search_type);
		w.one(encode_signs);
		w.one(polysemous_ht);
		return;
	}
	}
	throw_faiss("void faiss::write_index(const faiss::Index*, const char*)", "faiss/impl/index_write.cpp",
	            "don't know how to serialize this type of index");
}

void read_image(Reader &r, HostIndex &h);
// read_ivf_header: header, nlist, nprobe, the quantizer, the direct map (read and dropped)
void read_ivf_header(Reader &r, HostIndex &h) {
	read_header(r, h);
	uint64_t nlist = 0, nprobe = 0;
	r.one(nlist);
	r.one(nprobe);
	h.nlist = (int64_t)nlist;
	h.nprobe = (int64_t)nprobe;
	h.sub.reset(new HostIndex);
	read_image(r, *h.sub);
	char dm_type = 0;
	r.one(dm_type);
	std::vector<int64_t> dm_array;
	r.vec(dm_array);
	if (dm_type == 2) { // DirectMap::Hashtable: vector of (idx_t, idx_t) pairs
		std::vector<int64_t> pairs;
		uint64_t n = 0;
		r.one(n);
		if (n > ((uint64_t)1 << 40) / (2 * sizeof(int64_t))) // same bound READVECTOR applies
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "Error: 'size >= 0 && size < (uint64_t{1} << 40)' failed in %s", r.name);
		pairs.resize((size_t)n * 2);
		r.raw(pairs.data(), pairs.size() * sizeof(int64_t));
	}
}
// read_InvertedLists (ArrayInvertedLists) of rows of code_size bytes
template <typename T>
void read_lists(Reader &r, const char *kind, uint64_t nlist, uint64_t code_size, std::vector<std::vector<int64_t>> &ids,
                std::vector<std::vector<T>> &codes) {
	uint32_t il = 0;
	r.one(il);
	ids.assign((size_t)nlist, {});
	codes.assign((size_t)nlist, {});
	if (il == fourcc("il00")) // no inverted lists stored
		return;
	if (il != fourcc("ilar"))
		throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
		            "read_InvertedLists: unsupported invlist type (only ArrayInvertedLists is implemented)");
	uint64_t nl2 = 0, cs2 = 0;
	r.one(nl2);
	r.one(cs2);
	if (nl2 != nlist || cs2 != code_size)
		throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
		            "inverted lists do not match the %s header", kind);
	uint32_t list_type = 0;
	r.one(list_type);
	std::vector<uint64_t> sizes((size_t)nlist, 0), tmp;
	r.vec(tmp);
	if (list_type == fourcc("full")) {
		if (tmp.size() != nlist)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "Error: 'sizes.size() == nlist' failed");
		sizes = tmp;
	} else if (list_type == fourcc("sprs")) {
		for (size_t j = 0; j + 1 < tmp.size(); j += 2) {
			if (tmp[j] >= nlist)
				throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
				            "sparse list number out of range");
			sizes[(size_t)tmp[j]] = tmp[j + 1];
		}
	} else {
		throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
		            "list_type %ud not recognized", list_type);
	}
	for (size_t i = 0; i < (size_t)nlist; i++) {
		if (!sizes[i])
			continue;
		if (sizes[i] > ((uint64_t)1 << 40) / code_size)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "inverted list %zu: size %llu out of range in %s", i, (unsigned long long)sizes[i], r.name);
		codes[i].resize((size_t)(sizes[i] * code_size / sizeof(T)));
		ids[i].resize((size_t)sizes[i]);
		r.raw(codes[i].data(), codes[i].size() * sizeof(T));
		r.raw(ids[i].data(), ids[i].size() * sizeof(int64_t));
	}
}

void read_image(Reader &r, HostIndex &h) {
	uint32_t cc = 0;
	r.one(cc);
	if (cc == fourcc("IxFI") || cc == fourcc("IxF2") || cc == fourcc("IxFl")) {
		h.kind = MVS_KIND_FLAT;
		read_header(r, h);
		r.vec(h.rows);
		if ((int64_t)h.rows.size() != h.ntotal * h.d)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "Error: 'idxf->codes.size() == idxf->ntotal * idxf->code_size' failed");
		return;
	}
	if (cc == fourcc("IxMp") || cc == fourcc("IxM2")) {
		h.kind = MVS_KIND_IDMAP;
		h.idmap2 = cc == fourcc("IxM2");
		read_header(r, h);
		h.sub.reset(new HostIndex);
		read_image(r, *h.sub);
		r.vec(h.ids);
		return;
	}
	if (cc == fourcc("IwFl")) {
		h.kind = MVS_KIND_IVFFLAT;
		read_ivf_header(r, h);
		read_lists(r, "IVFFlat", (uint64_t)h.nlist, (uint64_t)h.d * sizeof(float), h.list_ids, h.list_codes);
		return;
	}
	if (cc == fourcc("IwPQ") || cc == fourcc("IwQR")) {
		if (cc == fourcc("IwQR"))
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "Index type \"IwQR\" (IndexIVFPQR, IVFPQ with a refinement stage) is not implemented on the MI355X path");
		h.kind = MVS_KIND_IVFPQ;
		read_ivf_header(r, h);
		uint8_t by_residual = 0;
		uint64_t code_size = 0, d = 0, M = 0, nbits = 0;
		r.one(by_residual);
		r.one(code_size);
		r.one(d);
		r.one(M);
		r.one(nbits);
		if (!by_residual)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "IndexIVFPQ with by_residual = 0 is not implemented on the MI355X path");
		if (d != (uint64_t)h.d || M == 0 || M > d || nbits != 8 || code_size != M)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "IndexIVFPQ with d = %llu, M = %llu, nbits = %llu, code_size = %llu is not implemented on the MI355X path (8 bits per code only)",
			            (unsigned long long)d, (unsigned long long)M, (unsigned long long)nbits, (unsigned long long)code_size);
		h.pq_M = (int)M;
		r.vec(h.pq_centroids);
		read_lists(r, "IVFPQ", (uint64_t)h.nlist, code_size, h.list_ids, h.list_bytes);
		return;
	}
	if (cc == fourcc("IxSQ")) {
		h.kind = MVS_KIND_SQ;
		read_header(r, h);
		read_sq_block(r, h, "IndexScalarQuantizer");
		r.vec(h.sq_codes);
		if ((int64_t)h.sq_codes.size() != h.ntotal * (int64_t)h.d)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "Error: 'idxs->codes.size() == idxs->ntotal * idxs->code_size' failed");
		return;
	}
	if (cc == fourcc("IwSq")) {
		h.kind = MVS_KIND_IVFSQ;
		read_ivf_header(r, h);
		read_sq_block(r, h, "IndexIVFScalarQuantizer");
		uint64_t code_size = 0;
		uint8_t by_residual = 0;
		r.one(code_size);
		r.one(by_residual);
		if (!by_residual)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "IndexIVFScalarQuantizer with by_residual = 0 is not implemented on the MI355X path");
		if (code_size != (uint64_t)h.d)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "IndexIVFScalarQuantizer with d = %d, code_size = %llu is not implemented on the MI355X path (one byte per component only)",
			            h.d, (unsigned long long)code_size);
		read_lists(r, "IVFSQ", (uint64_t)h.nlist, code_size, h.list_ids, h.list_bytes);
		return;
	}
	if (cc == fourcc("IHNf") || cc == fourcc("IHNs")) {
		h.kind = cc == fourcc("IHNs") ? MVS_KIND_HNSWSQ : MVS_KIND_HNSW;
		read_header(r, h);
		r.vec(h.assign_probas);
		r.vec(h.cum_nneighbor_per_level);
		r.vec(h.levels);
		r.vec(h.offsets);
		r.vec(h.neighbors);
		r.one(h.entry_point);
		int32_t ml = 0, efc = 0, efs = 0, upper_beam = 0;
		r.one(ml);
		r.one(efc);
		r.one(efs);
		r.one(upper_beam);
		h.max_level = ml;
		h.efConstruction = efc;
		h.efSearch = efs;
		h.sub.reset(new HostIndex);
		read_image(r, *h.sub);
		if (cc == fourcc("IHNs") && h.sub->kind != MVS_KIND_SQ)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "Index type \"IHNs\" (IndexHNSWSQ) whose storage is not an IndexScalarQuantizer (\"IxSQ\") is not implemented on the MI355X path");
		if (cc == fourcc("IHNf") && h.sub->kind == MVS_KIND_SQ)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "Index type \"IHNf\" (IndexHNSWFlat) whose storage is an IndexScalarQuantizer (\"IxSQ\") is not implemented on the MI355X path");
		return;
	}
	if (cc == fourcc("IxRF")) {
		h.kind = MVS_KIND_REFINE;
		read_header(r, h);
		h.sub.reset(new HostIndex);
		read_image(r, *h.sub);
		h.sub2.reset(new HostIndex);
		read_image(r, *h.sub2);
		r.one(h.k_factor);
		return; // (what the two sub-indexes must agree on is checked by refine_from_host, csrc/refine.hip)
	}
	if (cc == fourcc("IxPT")) {
		h.kind = MVS_KIND_PRETRANSFORM;
		read_header(r, h);
		int32_t nt = 0;
		r.one(nt);
		if (nt < 1 || nt > 4)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "IndexPreTransform with a chain of %d transforms is not implemented on the MI355X path (1 to 4)", nt);
		for (int i = 0; i < nt; ++i) {
			HostTransform t;
			uint32_t tc = 0;
			r.one(tc);
			if (tc == fourcc("VNrm")) {
				t.type = MVS_VT_NORM;
				r.one(t.norm);
			} else if (tc == fourcc("LTra") || tc == fourcc("rrot") || tc == fourcc("PCAm") || tc == fourcc("PcAm")) {
				t.type = MVS_VT_LINEAR;
				if (tc == fourcc("PCAm") || tc == fourcc("PcAm")) {
					t.type = MVS_VT_PCA;
					r.one(t.eigen_power);
					if (tc == fourcc("PcAm"))
						r.one(t.epsilon);
					uint8_t rr = 0;
					r.one(rr);
					t.random_rotation = rr != 0;
					r.one(t.balanced_bins);
					r.vec(t.mean);
					r.vec(t.eigenvalues);
					r.vec(t.PCAMat);
				}
				uint8_t hb = 0;
				r.one(hb);
				t.have_bias = hb != 0;
				r.vec(t.A);
				r.vec(t.b);
			} else {
				char tt[5] = {(char)(tc & 0xff), (char)((tc >> 8) & 0xff), (char)((tc >> 16) & 0xff), (char)((tc >> 24) & 0xff), 0};
				for (char &c : tt)
					if (c && (c < 32 || c > 126))
						c = '?';
				throw_faiss("faiss::VectorTransform* faiss::read_VectorTransform(faiss::IOReader*)", "faiss/impl/index_read.cpp",
				            "VectorTransform type 0x%08x (\"%s\") is not implemented on the MI355X path (\"LTra\", \"rrot\", \"PCAm\", \"PcAm\" and "
				            "\"VNrm\" only)", tc, tt);
			}
			int32_t di = 0, dout = 0;
			uint8_t tr = 0;
			r.one(di);
			r.one(dout);
			r.one(tr);
			t.d_in = di, t.d_out = dout, t.is_trained = tr != 0;
			h.chain.push_back(std::move(t));
		}
		h.sub.reset(new HostIndex);
		read_image(r, *h.sub);
		return; // (what the chain and the sub-index must agree on is checked by pretransform_from_host, csrc/pretransform.hip)
	}
	if (cc == fourcc("IxPq")) {
		h.kind = MVS_KIND_PQ;
		read_header(r, h);
		uint64_t d = 0, M = 0, nbits = 0;
		r.one(d);
		r.one(M);
		r.one(nbits);
		if (d != (uint64_t)h.d || M == 0 || M > d || nbits != 8)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "IndexPQ with d = %llu, M = %llu, nbits = %llu is not implemented on the MI355X path (8 bits per code only)",
			            (unsigned long long)d, (unsigned long long)M, (unsigned long long)nbits);
		h.pq_M = (int)M;
		r.vec(h.pq_centroids);
		r.vec(h.pq_codes);
		if ((int64_t)h.pq_codes.size() != h.ntotal * (int64_t)M)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "Error: 'idxp->codes.size() == idxp->ntotal * idxp->code_size' failed");
		int32_t search_type = 0, polysemous_ht = 0;
		uint8_t encode_signs = 0;
		r.one(search_type);
		r.one(encode_signs);
		r.one(polysemous_ht);
		if (search_type != 0)
			throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
			            "IndexPQ search_type %d (polysemous / Hamming search) is not implemented on the MI355X path", search_type);
		return;
	}
	char txt[5] = {(char)(cc & 0xff), (char)((cc >> 8) & 0xff), (char)((cc >> 16) & 0xff), (char)((cc >> 24) & 0xff), 0};
	for (char &c : txt)
		if (c && (c < 32 || c > 126))
			c = '?';
	throw_faiss("faiss::Index* faiss::read_index(const char*, int)", "faiss/impl/index_read.cpp",
	            "Index type 0x%08x (\"%s\") not recognized or not implemented on the MI355X path", cc, txt);
}

} // namespace

void write_index_file(IndexBase *ix, const char *filename) {
	HostIndex h;
	ix->to_host(h);
	FILE *f = fopen(filename, "wb");
	if (!f)
		throw_faiss("faiss::FileIOWriter::FileIOWriter(const char*)", "faiss/impl/io.cpp",
		            "could not open %s for writing: %s", filename, strerror(errno));
	Writer w {f, filename};
	try {
		write_image(w, h);
	} catch (...) {
		fclose(f);
		throw;
	}
	if (fclose(f) != 0)
		throw_faiss("faiss::FileIOWriter::~FileIOWriter()", "faiss/impl/io.cpp", "file %s close error: %s", filename,
		            strerror(errno));
}

IndexBase *read_index_file(const char *filename) {
	FILE *f = fopen(filename, "rb");
	if (!f)
		throw_faiss("faiss::FileIOReader::FileIOReader(const char*)", "faiss/impl/io.cpp",
		            "could not open %s for reading: %s", filename, strerror(errno));
	HostIndex h;
	Reader r {f, filename};
	try {
		read_image(r, h);
	} catch (...) {
		fclose(f);
		throw;
	}
	fclose(f);
	// env MVS_DEVICES=0,1,...: the loaded index is spread over those devices (csrc/sharded.hip)
	const std::vector<int> devs = shard_devices_from_env();
	if (devs.size() > 1)
		return shard_from_host(h, devs);
	return index_from_host(h, -1);
}

} // namespace mvs
