// host/boundary_driver.cpp -- stand-alone driver that talks to the MI355X path EXACTLY the way the reference's glue
// does, through the faiss:: adaptor (compat/faiss/*.h): DuckDB itself is not available in this image, so this file
// reproduces the call patterns of /root/reference/src/faiss_extension.cpp around the FAISS boundary --
//   CreateFunction        :146-164   index_factory, needs_training = !is_trained
//   AddFunction           :475-547   <= 2048-row DataChunks from several worker threads, faiss_lock, error text
//   AddFinaliseFunction   :549-615   last thread out trains on ALL rows, then adds the rows not yet added
//   searchIntoVector      :621-666   new[] result arrays, faiss_lock, search, scatter into (rank,label,distance)
//   createSearchParameters:668-727   IDMap recursion, SearchParametersIVF/HNSW, selector
//   MoveToGPUFunction     gpu.cpp:34-63
// and prints the result rows so that tests/test_boundary_driver_gpu.py can compare them with the reference's
// golden vectors (test/sql/faiss.test, faiss3.test, faiss4.test, faiss7.test).
//
//   boundary_driver golden <training.csv> <queries.csv>
//   boundary_driver ingest <n> <d> <threads> [index]  (concurrent DataChunk ingest + self-query check; index = factory
//                                                      string, default "IDMap,Flat"; IVF, PQ, SQ8 and "...,RFlat" train in AddFinalise on all rows)
//   boundary_driver ivfpq <n> <d>                     (IDMap,IVF4,PQ4: the glue's IndexIVF cast and its nprobe)
//   boundary_driver linkrate                          (host -> device copy rate of this box: pinned and pageable)
//   boundary_driver range <rows> <d> <nq> <index>     (Index::range_search into a RangeSearchResult, checked against search)
//   boundary_driver pretransform <d> <n> <nq> <k>     (PCA8,Flat / L2norm,Flat / IDMap,PCAW8,IVF4,Flat: factory -> train -> add -> search through
//                                                      faiss::IndexPreTransform; prints labels and distance bits per query)
#include "faiss/Index.h"
#include "faiss/IndexBinary.h"
#include "faiss/IndexBinaryFlat.h"
#include "faiss/IndexHNSW.h"
#include "faiss/IndexIDMap.h"
#include "faiss/IndexIVF.h"
#include "faiss/IndexPreTransform.h"
#include "faiss/IndexRefine.h"
#include "faiss/gpu/GpuCloner.h"
#include "faiss/gpu/StandardGpuResources.h"
#include "faiss/index_factory.h"
#include "faiss/index_io.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <fstream>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

namespace {

constexpr size_t STANDARD_VECTOR_SIZE = 2048; // DuckDB DataChunk capacity

// FaissIndexEntry (src/include/index.hpp:12-56), reduced to what the path touches
struct IndexEntry {
	std::unique_ptr<std::mutex> faiss_lock {new std::mutex()};
	std::unique_ptr<faiss::Index> index;
	bool needs_training = true;
	bool custom_labels = false;
	std::atomic<uint64_t> currently_adding {0};
	std::unique_ptr<std::mutex> add_lock {new std::mutex()};
	std::vector<float> add_data;
	std::vector<faiss::idx_t> add_labels;
	size_t size = 0, added = 0;
};

struct InvalidInput : std::runtime_error {
	using std::runtime_error::runtime_error;
};

// CreateFunction :146-164 (default metric INNER_PRODUCT :105)
std::unique_ptr<IndexEntry> create(int d, const std::string &desc, faiss::MetricType metric = faiss::METRIC_INNER_PRODUCT) {
	auto e = std::make_unique<IndexEntry>();
	e->index.reset(faiss::index_factory(d, desc.c_str(), metric));
	e->needs_training = !e->index->is_trained;
	return e;
}

// AddFunction :475-547 for one DataChunk
// MVS_INGEST_PROFILE=1: the duration of every add call under the lock (where does an ingest's time go: the steady calls or the few
// that grow the device buffers)
static std::vector<double> g_add_us;
static const bool g_add_profile = getenv("MVS_INGEST_PROFILE") != nullptr;
void add_chunk(IndexEntry &entry, size_t n, const float *x, const faiss::idx_t *ids) {
	if (!entry.needs_training) {
		entry.faiss_lock->lock();
		try {
			const auto t0 = std::chrono::steady_clock::now();
			if (entry.custom_labels)
				entry.index->add_with_ids((faiss::idx_t)n, x, ids);
			else
				entry.index->add((faiss::idx_t)n, x);
			if (g_add_profile)
				g_add_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
		} catch (faiss::FaissException exception) {
			entry.faiss_lock->unlock();
			std::string msg = exception.msg;
			if (msg.find("add_with_ids not implemented for this type of index") != std::string::npos)
				throw InvalidInput("Unable to add data: This type of index does not support adding with IDs. "
				                   "Consider prefixing the index string with IDMap when creating the index.");
			throw InvalidInput(std::string("Unable to add data: ") + exception.what());
		}
		entry.faiss_lock->unlock();
		return;
	}
	std::lock_guard<std::mutex> g(*entry.add_lock);
	entry.add_data.insert(entry.add_data.end(), x, x + n * entry.index->d);
	if (entry.custom_labels)
		entry.add_labels.insert(entry.add_labels.end(), ids, ids + n);
	entry.size += n;
}

// AddFinaliseFunction :549-615
void add_finalise(IndexEntry &entry) {
	size_t total, added;
	{
		std::lock_guard<std::mutex> g(*entry.add_lock);
		entry.currently_adding--;
		if (entry.currently_adding != 0)
			return;
		total = entry.size;
		added = entry.added;
		if (added == total)
			return;
		entry.added = total;
	}
	if (entry.add_data.empty())
		return;
	std::lock_guard<std::mutex> g(*entry.faiss_lock);
	try {
		entry.index->train((faiss::idx_t)total, entry.add_data.data());
	} catch (faiss::FaissException exception) {
		std::string msg = exception.msg;
		if (msg.find("should be at least as large as number of clusters") != std::string::npos)
			throw InvalidInput("Index needs to be trained, but amount of datapoints is too small. Considere adding more "
			                   "data. (" + msg + ")");
		throw InvalidInput("Error occured while training index: " + msg);
	}
	const faiss::idx_t nnew = (faiss::idx_t)(total - added);
	const float *xnew = entry.add_data.data() + added * entry.index->d;
	if (entry.custom_labels)
		entry.index->add_with_ids(nnew, xnew, entry.add_labels.data() + added);
	else
		entry.index->add(nnew, xnew);
	entry.needs_training = !entry.index->is_trained;
}

// faiss_add((SELECT [id,] vec ...), name): chunks of <= 2048 rows pulled by `nthreads` workers
void faiss_add(IndexEntry &entry, size_t n, const float *x, const faiss::idx_t *ids, int nthreads) {
	entry.custom_labels = ids != nullptr;
	const size_t d = (size_t)entry.index->d;
	const size_t nchunks = (n + STANDARD_VECTOR_SIZE - 1) / STANDARD_VECTOR_SIZE;
	std::atomic<size_t> next {0};
	std::vector<std::thread> workers;
	std::mutex err_lock;
	std::string err;
	entry.currently_adding += nthreads; // AddLocalInit per worker :462-473
	for (int t = 0; t < nthreads; ++t)
		workers.emplace_back([&] {
			try {
				std::vector<float> chunk;
				std::vector<faiss::idx_t> idc;
				for (;;) {
					size_t c = next++;
					if (c >= nchunks)
						break;
					size_t r0 = c * STANDARD_VECTOR_SIZE, nr = std::min(STANDARD_VECTOR_SIZE, n - r0);
					// the chunk lives in a buffer that is only valid during the call -- the worker's DataChunk, whose vector buffers
					// DuckDB REUSES from chunk to chunk (a fresh 1 MB allocation per chunk costs a page-fault storm that an
					// operator pipeline does not have: 8 threads of them slowed every add call from 39 to 60 us)
					chunk.assign(x + r0 * d, x + (r0 + nr) * d);
					if (ids)
						idc.assign(ids + r0, ids + r0 + nr);
					add_chunk(entry, nr, chunk.data(), ids ? idc.data() : nullptr);
				}
				add_finalise(entry);
			} catch (const std::exception &e) {
				std::lock_guard<std::mutex> g(err_lock);
				err = e.what();
			}
		});
	for (auto &w : workers)
		w.join();
	if (!err.empty())
		throw InvalidInput(err);
}

// innerCreateSearchParameters :668-721
std::vector<std::shared_ptr<faiss::SearchParameters>> create_search_parameters(faiss::Index *index, faiss::IDSelector *sel,
                                                                               int nprobe, int efSearch) {
	if (auto idmap = dynamic_cast<faiss::IndexIDMap *>(index))
		return create_search_parameters(idmap->index, sel, nprobe, efSearch);
	if (auto ivf = dynamic_cast<faiss::IndexIVF *>(index)) {
		auto p = std::make_shared<faiss::SearchParametersIVF>();
		p->sel = sel;
		auto ret = create_search_parameters(ivf->quantizer, nullptr, 0, 0);
		p->quantizer_params = ret[0].get();
		if (nprobe > 0)
			p->nprobe = (size_t)nprobe;
		ret.insert(ret.begin(), p);
		return ret;
	}
	if (dynamic_cast<faiss::IndexHNSW *>(index)) {
		auto p = std::make_shared<faiss::SearchParametersHNSW>();
		p->sel = sel;
		if (efSearch > 0)
			p->efSearch = efSearch;
		return {p};
	}
	if (dynamic_cast<faiss::IndexPQ *>(index))
		return {std::make_shared<faiss::SearchParametersPQ>()};
	auto p = std::make_shared<faiss::SearchParameters>();
	p->sel = sel;
	return {p};
}

struct ResultRow {
	int rank;
	int64_t label;
	float distance;
};
// searchIntoVector :621-666
std::vector<ResultRow> search_into_vector(IndexEntry &entry, size_t nq, const float *x, size_t k,
                                          faiss::SearchParameters *params) {
	std::unique_ptr<faiss::idx_t[]> labels(new faiss::idx_t[nq * k]);
	std::unique_ptr<float[]> distances(new float[nq * k]);
	entry.faiss_lock->lock();
	try {
		entry.index->search((faiss::idx_t)nq, x, (faiss::idx_t)k, distances.get(), labels.get(), params);
	} catch (faiss::FaissException exception) {
		entry.faiss_lock->unlock();
		throw InvalidInput("Error occured while searching: " + exception.msg);
	}
	entry.faiss_lock->unlock();
	std::vector<ResultRow> out(nq * k);
	for (size_t r = 0; r < nq; ++r)
		for (size_t j = 0; j < k; ++j)
			out[r * k + j] = {(int)j, labels[r * k + j], distances[r * k + j]};
	return out;
}
// faiss_search over a column of queries: one call per DataChunk (<= 2048 rows)
std::vector<ResultRow> faiss_search(IndexEntry &entry, size_t nq, const float *x, size_t k, faiss::IDSelector *sel = nullptr,
                                    int nprobe = 0, int efSearch = 0) {
	std::vector<ResultRow> all;
	const size_t d = (size_t)entry.index->d;
	for (size_t q0 = 0; q0 < nq; q0 += STANDARD_VECTOR_SIZE) {
		size_t nn = std::min(STANDARD_VECTOR_SIZE, nq - q0);
		auto params = create_search_parameters(entry.index.get(), sel, nprobe, efSearch);
		auto rows = search_into_vector(entry, nn, x + q0 * d, k, params[0].get());
		all.insert(all.end(), rows.begin(), rows.end());
	}
	return all;
}

bool read_csv(const char *path, std::vector<faiss::idx_t> &ids, std::vector<float> &vecs, int &d) {
	std::ifstream f(path);
	if (!f)
		return false;
	std::string line;
	d = 0;
	while (std::getline(f, line)) {
		if (line.empty())
			continue;
		std::stringstream ss(line);
		std::string cell;
		int col = 0;
		while (std::getline(ss, cell, ',')) {
			if (col == 0)
				ids.push_back((faiss::idx_t)std::stoll(cell));
			else
				vecs.push_back((float)std::stod(cell)); // LIST<DOUBLE> -> FLOAT cast, :292-293
			++col;
		}
		d = col - 1;
	}
	return true;
}

void print_rows(const char *tag, const std::vector<ResultRow> &rows) {
	for (auto &r : rows)
		printf("%s\t%d\t%lld\t%.9g\n", tag, r.rank, (long long)r.label, r.distance);
}

int run_golden(const char *train_csv, const char *query_csv) {
	std::vector<faiss::idx_t> ids, qids;
	std::vector<float> xb, xq;
	int d = 0, dq = 0;
	if (!read_csv(train_csv, ids, xb, d) || !read_csv(query_csv, qids, xq, dq) || d != dq) {
		fprintf(stderr, "cannot read fixtures\n");
		return 2;
	}
	const size_t n = ids.size(), nq = qids.size();
	{ // test/sql/faiss.test: Flat, no ids
		auto e = create(d, "Flat");
		faiss_add(*e, n, xb.data(), nullptr, 1);
		print_rows("flat", faiss_search(*e, nq, xq.data(), 2));
	}
	{ // test/sql/faiss3.test: IDMap,Flat + bitmap filter 'column0>100'
		auto e = create(d, "IDMap,Flat");
		faiss_add(*e, n, xb.data(), ids.data(), 3);
		print_rows("idmap", faiss_search(*e, nq, xq.data(), 2));
		faiss::idx_t maxid = 0;
		for (auto v : ids)
			maxid = std::max(maxid, v);
		std::vector<uint8_t> mask((size_t)maxid / 8 + 1, 0); // :765-767
		for (auto v : ids)
			if (v > 100)
				mask[(size_t)v >> 3] |= (uint8_t)(1u << (v & 7));
		faiss::IDSelectorBitmap sel(mask.size(), mask.data()); // :959
		print_rows("filter", faiss_search(*e, nq, xq.data(), 2, &sel));
		std::vector<faiss::idx_t> keep;
		for (auto v : ids)
			if (v > 100)
				keep.push_back(v);
		faiss::IDSelectorBatch selb(keep.size(), keep.data()); // :1008
		print_rows("filterset", faiss_search(*e, nq, xq.data(), 2, &selb));
	}
	{ // test/sql/faiss4.test / faiss6.test: ids on a plain Flat index
		auto e = create(d, "Flat", faiss::METRIC_L2);
		try {
			faiss_add(*e, n, xb.data(), ids.data(), 1);
			printf("error\tnone\n");
		} catch (const InvalidInput &ex) {
			printf("error\t%s\n", ex.what());
		}
		faiss_add(*e, n, xb.data(), nullptr, 2);
		printf("ntotal\t%lld\n", (long long)e->index->ntotal);
	}
	{ // test/sql/faiss7.test: N = 1 < k = 2 with a filter that excludes the only row
		auto e = create(2, "IDMap,Flat");
		float v[2] = {0.0040321066f, 0.023423655f};
		faiss::idx_t id = 231;
		faiss_add(*e, 1, v, &id, 1);
		float q[2] = {-0.04529257f, 0.024853613f};
		uint8_t mask[29] = {0};
		faiss::IDSelectorBitmap sel(sizeof mask, mask);
		print_rows("small", faiss_search(*e, 1, q, 2));
		print_rows("smallfilter", faiss_search(*e, 1, q, 2, &sel));
	}
	{ // faiss_to_gpu(name, device): src/gpu/gpu.cpp:34-63
		auto e = create(d, "IDMap,Flat");
		faiss_add(*e, n, xb.data(), ids.data(), 2);
		faiss::gpu::StandardGpuResources res;
		e->index.reset(faiss::gpu::index_cpu_to_gpu(&res, 0, e->index.get()));
		print_rows("togpu", faiss_search(*e, nq, xq.data(), 2));
		try {
			e->index.reset(faiss::gpu::index_cpu_to_gpu(&res, 4096, e->index.get()));
			printf("gpuerror\tnone\n");
		} catch (faiss::FaissException exception) {
			printf("gpuerror\t%s\n", exception.msg.find("Invalid GPU device") != std::string::npos ? "Invalid GPU index"
			                                                                                         : exception.msg.c_str());
		}
	}
	return 0;
}

// concurrent ingest the way DuckDB drives faiss_add for a large table, then self-queries
int run_ingest(size_t n, int d, int threads, const char *desc = "IDMap,Flat") {
	std::vector<float> xb(n * (size_t)d);
	uint64_t s = 88172645463325252ull;
	for (auto &v : xb) {
		s ^= s << 13;
		s ^= s >> 7;
		s ^= s << 17;
		v = (float)(s >> 40) * (1.0f / 16777216.0f);
	}
	std::vector<faiss::idx_t> ids(n);
	for (size_t i = 0; i < n; ++i)
		ids[i] = (faiss::idx_t)(1000000 + 7 * i);
	const bool with_ids = !strncmp(desc, "IDMap", 5);
	auto e = create(d, desc, faiss::METRIC_L2);
	const auto t0 = std::chrono::steady_clock::now();
	faiss_add(*e, n, xb.data(), with_ids ? ids.data() : nullptr, threads);
	// add() returns while the last H2D copies are still in flight: a 1-query search drains the index's stream
	(void)faiss_search(*e, 1, xb.data(), 1);
	const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	if (g_add_profile && !g_add_us.empty()) {
		std::vector<double> v = g_add_us;
		std::sort(v.begin(), v.end());
		double tot = 0, slow = 0;
		size_t nslow = 0;
		for (double u : v) {
			tot += u;
			if (u > 500.0)
				slow += u, ++nslow;
		}
		printf("ingestprofile\t%zu add calls: %.1f ms under the lock of %.1f ms; median %.1f us, p90 %.1f us; %zu calls over 500 us = %.1f ms\n",
		       v.size(), tot / 1e3, sec * 1e3, v[v.size() / 2], v[v.size() * 9 / 10], nslow, slow / 1e3);
	}
	printf("ingestrate\t%.0f rows/s (%s: %zu rows x %d dims in %zu add calls of <= 2048 rows from %d threads: %.3f s, %.2f GB/s "
	       "of row data)\n",
	       (double)n / sec, desc, n, d, (n + 2047) / 2048, threads, sec, (double)n * d * 4 / sec / 1e9);
	printf("ingestjson\t{\"index\": \"%s\", \"rows\": %zu, \"d\": %d, \"threads\": %d, \"seconds\": %.4f, \"rows_per_s\": %.0f, "
	       "\"GBps\": %.3f}\n",
	       desc, n, d, threads, sec, (double)n / sec, (double)n * d * 4 / sec / 1e9);
	if (strstr(desc, ",RFlat") || strstr(desc, ",Refine(")) {
		// "<base>,RFlat" the way the glue sees it: an IndexRefine under the IndexIDMap, which is NOT an IndexIVF (the cast at :675 fails on it
		// as on FAISS's class: no nprobe from SQL), and whose k_factor member, assigned on the wrapper, reaches the search -- with 64 base
		// candidates re-scored exactly every row finds itself at distance 0 in the one list its query probes
		faiss::Index *ix = e->index.get();
		if (auto idmap = dynamic_cast<faiss::IndexIDMap *>(ix))
			ix = idmap->index;
		auto *rf = dynamic_cast<faiss::IndexRefine *>(ix);
		const bool is_ivf = dynamic_cast<faiss::IndexIVF *>(ix) != nullptr;
		size_t okr = 0;
		const size_t nqr = std::min<size_t>(n, 512);
		if (rf && rf->base_index && rf->refine_index) {
			rf->k_factor = 64;
			auto rows = faiss_search(*e, nqr, xb.data(), 1);
			for (size_t i = 0; i < nqr; ++i)
				okr += (!with_ids || rows[i].label == ids[i]) && rows[i].distance == 0.f; // (without ids the label is the arrival number)
		}
		const bool okf = rf && !is_ivf && okr == nqr && (size_t)mvs_index_ntotal(rf->refine_index->handle) == n && (size_t)mvs_index_ntotal(rf->base_index->handle) == n;
		printf("refine\t%s IndexRefine=%d IndexIVF=%d k_factor=64: %zu/%zu self-queries at distance 0\n", okf ? "OK" : "FAIL", rf != nullptr, is_ivf,
		       okr, nqr);
		if (!okf)
			return 1;
	}
	if (!with_ids || strstr(desc, "HNSW") || strstr(desc, "IVF") || strstr(desc, "PQ") || strstr(desc, "SQ")) { // (approximate indexes: no self-query guarantee; the count is the check)
		const bool okc = (size_t)e->index->ntotal == n;
		printf("ingest\t%s ntotal=%lld, threads=%d\n", okc ? "OK" : "FAIL", (long long)e->index->ntotal, threads);
		return okc ? 0 : 1;
	}
	if ((size_t)e->index->ntotal != n) {
		printf("ingest\tFAIL ntotal %lld\n", (long long)e->index->ntotal);
		return 1;
	}
	// chunks arrive in nondeterministic order; every vector must still find itself under its own label
	const size_t nq = std::min<size_t>(n, 4096);
	auto rows = faiss_search(*e, nq, xb.data(), 1);
	size_t ok = 0;
	for (size_t i = 0; i < nq; ++i)
		ok += rows[i].label == ids[i] && rows[i].distance <= 1e-5f;
	printf("ingest\t%s %zu/%zu self-queries, ntotal=%lld, threads=%d\n", ok == nq ? "OK" : "FAIL", ok, nq,
	       (long long)e->index->ntotal, threads);
	return ok == nq ? 0 : 1;
}

// IDMap,IVF4,PQ4 the way the glue sees it: the cast of innerCreateSearchParameters (:675) must find an IndexIVF under the IndexIDMap --
// and the IndexPQ branch (:704) must not --, and the nprobe set there must reach the search: with k beyond one list's rows, nprobe = 1
// pads its result with -1 while nprobe = nlist fills it
int run_ivfpq(size_t n, int d) {
	std::vector<float> xb(n * (size_t)d);
	uint64_t s = 88172645463325252ull;
	for (auto &v : xb) {
		s ^= s << 13;
		s ^= s >> 7;
		s ^= s << 17;
		v = (float)(s >> 40) * (1.0f / 16777216.0f);
	}
	std::vector<faiss::idx_t> ids(n);
	for (size_t i = 0; i < n; ++i)
		ids[i] = (faiss::idx_t)(1000000 + 7 * i);
	auto e = create(d, "IDMap,IVF4,PQ4", faiss::METRIC_L2);
	faiss_add(*e, n, xb.data(), ids.data(), 1);
	auto *idmap = dynamic_cast<faiss::IndexIDMap *>(e->index.get());
	auto *ivf = idmap ? dynamic_cast<faiss::IndexIVF *>(idmap->index) : nullptr;
	const bool is_pq = idmap && dynamic_cast<faiss::IndexPQ *>(idmap->index) != nullptr;
	const size_t k = std::min<size_t>(n, 2048);
	size_t found1 = 0, found4 = 0;
	for (const auto &r : faiss_search(*e, 1, xb.data(), k, nullptr, 1))
		found1 += r.label >= 0;
	for (const auto &r : faiss_search(*e, 1, xb.data(), k, nullptr, 4))
		found4 += r.label >= 0;
	const bool ok = ivf && !is_pq && ivf->nlist == 4 && (size_t)e->index->ntotal == n && found1 > 0 && found1 < k && found4 == k;
	printf("ivfpq\t%s IndexIVF=%d IndexPQ=%d nlist=%zu ntotal=%lld nprobe=1: %zu of %zu slots, nprobe=4: %zu\n", ok ? "OK" : "FAIL", ivf != nullptr,
	       (int)is_pq, ivf ? ivf->nlist : (size_t)0, (long long)e->index->ntotal, found1, k, found4);
	return ok ? 0 : 1;
}

// Index::range_search through the faiss:: classes, L2: the radius is the median 10th-neighbour distance of the batch, and for every query
// the result must equal the entries of search(k = min(ntotal, 1024)) with a distance inside the radius, wherever fewer than k pass (then
// search has seen them all).  Range results come in row / list order, search results by distance: both are compared sorted by label.
int run_range(size_t n, int d, size_t nq, const char *desc) {
	std::vector<float> xb(n * (size_t)d), xq(nq * (size_t)d);
	uint64_t s = 0x9E3779B97F4A7C15ull;
	auto next = [&]() {
		s ^= s << 13;
		s ^= s >> 7;
		s ^= s << 17;
		return (float)(s >> 40) * (1.0f / 16777216.0f);
	};
	for (auto &v : xb)
		v = next();
	for (auto &v : xq)
		v = next();
	std::vector<faiss::idx_t> ids(n);
	for (size_t i = 0; i < n; ++i)
		ids[i] = (faiss::idx_t)(1000000 + 7 * i);
	const bool with_ids = !strncmp(desc, "IDMap", 5);
	auto e = create(d, desc, faiss::METRIC_L2);
	faiss_add(*e, n, xb.data(), with_ids ? ids.data() : nullptr, 2);
	const size_t k = std::min<size_t>((size_t)e->index->ntotal, 1024);
	if (k < 10 || nq == 0) {
		printf("RANGE FAIL needs at least 10 rows and one query\n");
		return 1;
	}
	auto params = create_search_parameters(e->index.get(), nullptr, 0, 0);
	auto rows = search_into_vector(*e, nq, xq.data(), k, params[0].get());
	std::vector<float> tenth;
	for (size_t q = 0; q < nq; ++q)
		if (rows[q * k + 9].label >= 0)
			tenth.push_back(rows[q * k + 9].distance);
	if (tenth.empty()) {
		printf("RANGE FAIL no query has ten neighbours\n");
		return 1;
	}
	std::sort(tenth.begin(), tenth.end());
	const float radius = tenth[tenth.size() / 2];
	faiss::RangeSearchResult res(nq);
	{
		std::lock_guard<std::mutex> g(*e->faiss_lock);
		e->index->range_search((faiss::idx_t)nq, xq.data(), radius, &res, params[0].get());
	}
	size_t bad = 0, checked = 0;
	for (size_t q = 0; q < nq; ++q) {
		std::vector<std::pair<faiss::idx_t, float>> want, got;
		for (size_t j = 0; j < k; ++j)
			if (rows[q * k + j].label >= 0 && rows[q * k + j].distance < radius)
				want.emplace_back(rows[q * k + j].label, rows[q * k + j].distance);
		if (want.size() >= k)
			continue; // (search may have cut the list off)
		for (size_t i = res.lims[q]; i < res.lims[q + 1]; ++i)
			got.emplace_back(res.labels[i], res.distances[i]);
		std::sort(want.begin(), want.end());
		std::sort(got.begin(), got.end());
		++checked;
		bad += want != got;
	}
	if (bad || !checked) {
		printf("RANGE FAIL %zu of %zu checked queries differ from search (radius %.9g, %zu hits)\n", bad, checked, radius, res.lims[nq]);
		return 1;
	}
	printf("RANGE OK %zu\n", res.lims[nq]);
	return 0;
}

// Index::remove_ids through the faiss:: classes, L2: every third row's id goes by an IDSelectorBatch (with a duplicate and an absent id), then
// a quarter of the id space by an IDSelectorBitmap.  The count, ntotal on the wrapper, on every wrapper of its chain and on the handle, and --
// for the kinds that compact stably (no IVF) -- a search against a fresh index of the survivors are checked; no result names a removed id.
int run_remove(size_t n, int d, size_t nq, const char *desc) {
	std::vector<float> xb(n * (size_t)d), xq(nq * (size_t)d);
	uint64_t s = 0x9E3779B97F4A7C15ull;
	auto next = [&]() {
		s ^= s << 13;
		s ^= s >> 7;
		s ^= s << 17;
		return (float)(s >> 40) * (1.0f / 16777216.0f);
	};
	for (auto &v : xb)
		v = next();
	for (auto &v : xq)
		v = next();
	const bool with_ids = !strncmp(desc, "IDMap", 5);
	const bool stable = strstr(desc, "IVF") == nullptr;
	std::vector<faiss::idx_t> ids(n);
	for (size_t i = 0; i < n; ++i)
		ids[i] = with_ids ? (faiss::idx_t)(100 + 3 * i) : (faiss::idx_t)i;
	auto e = create(d, desc, faiss::METRIC_L2);
	faiss_add(*e, n, xb.data(), with_ids ? ids.data() : nullptr, 1);
	if ((size_t)e->index->ntotal != n || n < 64 || nq == 0) {
		printf("REMOVE FAIL needs at least 64 rows and one query (ntotal %lld)\n", (long long)e->index->ntotal);
		return 1;
	}
	std::vector<char> gone(n, 0);
	std::vector<faiss::idx_t> batch;
	for (size_t i = 0; i < n; i += 3) {
		batch.push_back(ids[i]);
		gone[i] = 1;
	}
	batch.push_back(ids[0]);  // a duplicate
	batch.push_back(-12345); // not in the index
	size_t want = (n + 2) / 3, got = 0;
	{
		std::lock_guard<std::mutex> g(*e->faiss_lock);
		got = e->index->remove_ids(faiss::IDSelectorBatch(batch.size(), batch.data()));
	}
	// the ids the rows carry now: a bare Flat-like index renumbers its survivors, a bare IVF index and IDMap keep them
	auto current = [&](std::vector<faiss::idx_t> &cur, std::vector<size_t> &rows) {
		cur.clear(), rows.clear();
		for (size_t i = 0; i < n; ++i)
			if (!gone[i]) {
				cur.push_back(with_ids || !stable ? ids[i] : (faiss::idx_t)rows.size());
				rows.push_back(i);
			}
	};
	std::vector<faiss::idx_t> cur;
	std::vector<size_t> rows;
	current(cur, rows);
	bool ok = got == want && (size_t)e->index->ntotal == rows.size();
	// second removal: a bitmap over the ids as they are now (bits of every fourth surviving row)
	faiss::idx_t top = 0;
	for (auto v : cur)
		top = std::max(top, v);
	std::vector<uint8_t> bits((size_t)top / 8 + 1, 0);
	size_t want2 = 0;
	for (size_t j = 0; j < cur.size(); j += 4) {
		bits[(size_t)cur[j] >> 3] |= (uint8_t)(1u << (cur[j] & 7));
		gone[rows[j]] = 1;
		++want2;
	}
	size_t got2 = 0;
	{
		std::lock_guard<std::mutex> g(*e->faiss_lock);
		got2 = e->index->remove_ids(faiss::IDSelectorBitmap(bits.size(), bits.data()));
	}
	if (!stable && !with_ids) { // (ids kept: membership was by the ids of the first round)
		current(cur, rows);
	} else {
		std::vector<faiss::idx_t> c2;
		std::vector<size_t> r2;
		for (size_t j = 0; j < cur.size(); ++j)
			if (j % 4) {
				c2.push_back(with_ids || !stable ? cur[j] : (faiss::idx_t)r2.size());
				r2.push_back(rows[j]);
			}
		cur.swap(c2), rows.swap(r2);
	}
	ok = ok && got2 == want2 && (size_t)e->index->ntotal == rows.size() && mvs_index_ntotal(e->index->handle) == (int64_t)rows.size();
	if (auto *m = dynamic_cast<faiss::IndexIDMap *>(e->index.get()))
		ok = ok && m->index && (size_t)m->index->ntotal == rows.size() && mvs_index_ntotal(m->index->handle) == (int64_t)rows.size();
	const size_t k = std::min<size_t>(rows.size(), 10);
	auto params = create_search_parameters(e->index.get(), nullptr, 0, 0);
	auto res = search_into_vector(*e, nq, xq.data(), k, params[0].get());
	std::vector<faiss::idx_t> sorted_cur(cur);
	std::sort(sorted_cur.begin(), sorted_cur.end());
	size_t stale = 0, differ = 0;
	for (const auto &r : res)
		stale += r.label >= 0 && !std::binary_search(sorted_cur.begin(), sorted_cur.end(), r.label);
	if (stable) {
		std::vector<float> xs(rows.size() * (size_t)d);
		for (size_t j = 0; j < rows.size(); ++j)
			memcpy(&xs[j * (size_t)d], &xb[rows[j] * (size_t)d], (size_t)d * sizeof(float));
		auto f = create(d, desc, faiss::METRIC_L2);
		faiss_add(*f, rows.size(), xs.data(), with_ids ? cur.data() : nullptr, 1);
		auto fres = search_into_vector(*f, nq, xq.data(), k, params[0].get());
		for (size_t i = 0; i < res.size(); ++i)
			differ += res[i].label != fres[i].label || memcmp(&res[i].distance, &fres[i].distance, sizeof(float)) != 0;
	}
	if (!ok || stale || differ) {
		printf("REMOVE FAIL removed %zu (want %zu) and %zu (want %zu), ntotal %lld (want %zu), %zu stale labels, %zu entries differ from a fresh index\n", got,
		       want, got2, want2, (long long)e->index->ntotal, rows.size(), stale, differ);
		return 1;
	}
	printf("REMOVE OK %zu %zu %lld\n", got, got2, (long long)e->index->ntotal);
	return 0;
}

// The selector classes the glue does not build -- And(Range, Not(Batch)) -- through the faiss:: classes (compat/faiss/impl/IDSelector.h), which
// the adaptor flattens to one selector program: a filtered search and remove_ids must equal, bit for bit, the same calls given IDSelectorBatch of
// the ids the tree's own is_member admits, on a twin index
int run_selectors(size_t n, int d, size_t nq, const char *desc) {
	std::vector<float> xb(n * (size_t)d), xq(nq * (size_t)d);
	uint64_t s = 0x9E3779B97F4A7C15ull;
	auto next = [&]() {
		s ^= s << 13;
		s ^= s >> 7;
		s ^= s << 17;
		return (float)(s >> 40) * (1.0f / 16777216.0f);
	};
	for (auto &v : xb)
		v = next();
	for (auto &v : xq)
		v = next();
	const bool with_ids = !strncmp(desc, "IDMap", 5);
	std::vector<faiss::idx_t> ids(n);
	for (size_t i = 0; i < n; ++i)
		ids[i] = with_ids ? (faiss::idx_t)(100 + 3 * i) : (faiss::idx_t)i;
	auto e = create(d, desc, faiss::METRIC_L2), f = create(d, desc, faiss::METRIC_L2);
	faiss_add(*e, n, xb.data(), with_ids ? ids.data() : nullptr, 1);
	faiss_add(*f, n, xb.data(), with_ids ? ids.data() : nullptr, 1);
	if ((size_t)e->index->ntotal != n || n < 64 || nq == 0) {
		printf("SELECTORS FAIL needs at least 64 rows and one query (ntotal %lld)\n", (long long)e->index->ntotal);
		return 1;
	}
	std::vector<faiss::idx_t> excluded;
	for (size_t i = 0; i < n; i += 7)
		excluded.push_back(ids[i]);
	excluded.push_back(-12345); // not in the index
	faiss::IDSelectorRange range(ids[n / 4], ids[3 * n / 4]);
	faiss::IDSelectorBatch batch(excluded.size(), excluded.data());
	faiss::IDSelectorNot not_batch(&batch);
	faiss::IDSelectorAnd tree(&range, &not_batch);
	std::vector<faiss::idx_t> admitted;
	for (size_t i = 0; i < n; ++i)
		if (tree.is_member(ids[i]))
			admitted.push_back(ids[i]);
	faiss::IDSelectorBatch plain(admitted.size(), admitted.data());
	const size_t k = 10;
	auto compare = [&](faiss::IDSelector *a, faiss::IDSelector *b) {
		auto pa = create_search_parameters(e->index.get(), a, 4, 0), pb = create_search_parameters(f->index.get(), b, 4, 0);
		auto ra = search_into_vector(*e, nq, xq.data(), k, pa[0].get()), rb = search_into_vector(*f, nq, xq.data(), k, pb[0].get());
		size_t differ = 0;
		for (size_t i = 0; i < ra.size(); ++i)
			differ += ra[i].label != rb[i].label || memcmp(&ra[i].distance, &rb[i].distance, sizeof(float)) != 0;
		return differ;
	};
	const size_t differ_search = compare(&tree, &plain);
	size_t got = 0, want = 0;
	{
		std::lock_guard<std::mutex> g(*e->faiss_lock);
		got = e->index->remove_ids(tree);
	}
	{
		std::lock_guard<std::mutex> g(*f->faiss_lock);
		want = f->index->remove_ids(plain);
	}
	const size_t differ_after = compare(nullptr, nullptr);
	if (differ_search || differ_after || got != want || got != admitted.size() || e->index->ntotal != f->index->ntotal ||
	    (size_t)e->index->ntotal != n - admitted.size()) {
		printf("SELECTORS FAIL %zu search entries differ, %zu after remove_ids; removed %zu (the batch: %zu, admitted %zu), ntotal %lld / %lld\n", differ_search,
		       differ_after, got, want, admitted.size(), (long long)e->index->ntotal, (long long)f->index->ntotal);
		return 1;
	}
	printf("SELECTORS OK %s n %zu admitted %zu removed %zu ntotal %lld\n", desc, n, admitted.size(), got, (long long)e->index->ntotal);
	return 0;
}

// Index::merge_from through the faiss:: classes: the parallel build.  Two threads each fill a private index with one half of the rows -- no
// lock is shared on the add path --, the parts are merged under both locks, and the result must answer bit for bit like one index filled
// under the lock.  An IVF kind's parts take the whole's centroids (they must agree bit for bit: include/mi355_faiss.h "merge_from and
// copy_subset_to"); without IDMap its second part's implicit ids are shifted by add_id
int run_merge(size_t n, int d, size_t nq, const char *desc) {
	std::vector<float> xb(n * (size_t)d), xq(nq * (size_t)d);
	uint64_t s = 0xA0761D6478BD642Full;
	auto next = [&]() {
		s ^= s << 13;
		s ^= s >> 7;
		s ^= s << 17;
		return (float)(s >> 40) * (1.0f / 16777216.0f);
	};
	for (auto &v : xb)
		v = next();
	for (auto &v : xq)
		v = next();
	const bool with_ids = !strncmp(desc, "IDMap", 5);
	std::vector<faiss::idx_t> ids(n);
	for (size_t i = 0; i < n; ++i)
		ids[i] = with_ids ? (faiss::idx_t)(100 + 3 * i) : (faiss::idx_t)i;
	auto whole = create(d, desc, faiss::METRIC_L2);
	faiss_add(*whole, n, xb.data(), with_ids ? ids.data() : nullptr, 1);
	if ((size_t)whole->index->ntotal != n || n < 64 || nq == 0) {
		printf("MERGE FAIL needs at least 64 rows and one query (ntotal %lld)\n", (long long)whole->index->ntotal);
		return 1;
	}
	const int64_t nlist = mvs_index_ivf_nlist(whole->index->handle);
	std::vector<float> cent;
	if (nlist > 0) {
		cent.resize((size_t)nlist * (size_t)d);
		if (mvs_index_ivf_get_centroids(whole->index->handle, cent.data()))
			faiss::throw_last_error();
	}
	std::unique_ptr<IndexEntry> part[2];
	for (auto &p : part) {
		p = create(d, desc, faiss::METRIC_L2);
		if (nlist > 0 && mvs_index_ivf_set_centroids(p->index->handle, cent.data()))
			faiss::throw_last_error();
		p->index->refresh_chain();
		p->needs_training = !p->index->is_trained;
	}
	const size_t half = n / 2, row0[2] = {0, half}, rows[2] = {half, n - half};
	std::string err[2];
	std::thread worker[2];
	for (int t = 0; t < 2; ++t)
		worker[t] = std::thread([&, t] {
			try {
				faiss_add(*part[t], rows[t], &xb[row0[t] * (size_t)d], with_ids ? &ids[row0[t]] : nullptr, 1);
			} catch (const std::exception &e) {
				err[t] = e.what();
			}
		});
	for (auto &w : worker)
		w.join();
	if (!err[0].empty() || !err[1].empty()) {
		printf("MERGE FAIL a part could not be filled: %s %s\n", err[0].c_str(), err[1].c_str());
		return 1;
	}
	{
		std::lock(*part[0]->faiss_lock, *part[1]->faiss_lock);
		std::lock_guard<std::mutex> g0(*part[0]->faiss_lock, std::adopt_lock), g1(*part[1]->faiss_lock, std::adopt_lock);
		part[0]->index->check_compatible_for_merge(*part[1]->index);
		part[0]->index->merge_from(*part[1]->index, !with_ids && nlist > 0 ? (faiss::idx_t)half : 0);
	}
	bool ok = (size_t)part[0]->index->ntotal == n && mvs_index_ntotal(part[0]->index->handle) == (int64_t)n && part[1]->index->ntotal == 0 &&
	          mvs_index_ntotal(part[1]->index->handle) == 0 && part[1]->index->is_trained;
	if (auto *m = dynamic_cast<faiss::IndexIDMap *>(part[0]->index.get()))
		ok = ok && m->index && (size_t)m->index->ntotal == n;
	const size_t k = 10;
	auto pw = create_search_parameters(whole->index.get(), nullptr, 4, 0), pm = create_search_parameters(part[0]->index.get(), nullptr, 4, 0);
	auto rw = search_into_vector(*whole, nq, xq.data(), k, pw[0].get()), rm = search_into_vector(*part[0], nq, xq.data(), k, pm[0].get());
	size_t differ = 0;
	for (size_t i = 0; i < rw.size(); ++i)
		differ += rw[i].label != rm[i].label || memcmp(&rw[i].distance, &rm[i].distance, sizeof(float)) != 0;
	auto re = search_into_vector(*part[1], nq, xq.data(), k, create_search_parameters(part[1]->index.get(), nullptr, 4, 0)[0].get());
	size_t leftover = 0;
	for (const auto &r : re)
		leftover += r.label != -1;
	if (!ok || differ || leftover) {
		printf("MERGE FAIL ntotal %lld + %lld (want %zu + 0), %zu entries differ from the index filled under the lock, %zu labels from the emptied part\n",
		       (long long)part[0]->index->ntotal, (long long)part[1]->index->ntotal, n, differ, leftover);
		return 1;
	}
	printf("MERGE OK %s n %zu ntotal %lld\n", desc, n, (long long)part[0]->index->ntotal);
	return 0;
}

// Index::reconstruct, reconstruct_n, reconstruct_batch and search_and_reconstruct through the faiss:: classes, L2, over a kind that stores
// the f32 rows ("Flat", "IDMap,Flat", "IVF<n>,Flat", ...): every call must give the added row bit for bit, search_and_reconstruct the
// distances and labels of search with the rows of its labels, a padded slot a row of 0xFF bytes, and an absent key a FaissException
int run_reconstruct(size_t n, int d, size_t nq, const char *desc) {
	std::vector<float> xb(n * (size_t)d), xq(nq * (size_t)d);
	uint64_t s = 0xD1B54A32D192ED03ull;
	auto next = [&]() {
		s ^= s << 13;
		s ^= s >> 7;
		s ^= s << 17;
		return (float)(s >> 40) * (1.0f / 16777216.0f);
	};
	for (auto &v : xb)
		v = next();
	for (auto &v : xq)
		v = next();
	const bool with_ids = !strncmp(desc, "IDMap", 5);
	std::vector<faiss::idx_t> ids(n);
	for (size_t i = 0; i < n; ++i)
		ids[i] = with_ids ? (faiss::idx_t)(100 + 3 * i) : (faiss::idx_t)i;
	auto e = create(d, desc, faiss::METRIC_L2);
	faiss_add(*e, n, xb.data(), with_ids ? ids.data() : nullptr, 1);
	if ((size_t)e->index->ntotal != n || n < 8 || nq == 0) {
		printf("RECONSTRUCT FAIL needs at least 8 rows and one query (ntotal %lld)\n", (long long)e->index->ntotal);
		return 1;
	}
	const faiss::Index *ix = e->index.get();
	const size_t rb = (size_t)d * sizeof(float);
	size_t bad = 0;
	std::vector<float> one((size_t)d), all(n * (size_t)d);
	for (size_t i : {(size_t)0, n / 2, n - 1}) {
		ix->reconstruct(ids[i], one.data());
		bad += memcmp(one.data(), &xb[i * (size_t)d], rb) != 0;
	}
	std::vector<faiss::idx_t> keys;
	for (size_t j = 0; j < n; ++j)
		keys.push_back(ids[(j * 7 + 3) % n]);
	ix->reconstruct_batch((faiss::idx_t)keys.size(), keys.data(), all.data());
	for (size_t j = 0; j < n; ++j)
		bad += memcmp(&all[j * (size_t)d], &xb[((j * 7 + 3) % n) * (size_t)d], rb) != 0;
	if (!with_ids) { // (under IDMap the keys of a range are external ids, which these are not)
		ix->reconstruct_n(0, (faiss::idx_t)n, all.data());
		bad += memcmp(all.data(), xb.data(), n * rb) != 0;
	}
	bool refused = false;
	try {
		ix->reconstruct(-7, one.data());
	} catch (const faiss::FaissException &) {
		refused = true;
	}
	const size_t k = n + 2; // two padded slots per query
	auto params = create_search_parameters(e->index.get(), nullptr, 0, 0);
	std::vector<float> D(nq * k), D2(nq * k), R(nq * k * (size_t)d);
	std::vector<faiss::idx_t> I(nq * k), I2(nq * k);
	{
		std::lock_guard<std::mutex> g(*e->faiss_lock);
		ix->search((faiss::idx_t)nq, xq.data(), (faiss::idx_t)k, D.data(), I.data(), params[0].get());
		ix->search_and_reconstruct((faiss::idx_t)nq, xq.data(), (faiss::idx_t)k, D2.data(), I2.data(), R.data(), params[0].get());
	}
	size_t differ = memcmp(D.data(), D2.data(), D.size() * sizeof(float)) != 0 || memcmp(I.data(), I2.data(), I.size() * sizeof(faiss::idx_t)) != 0;
	size_t padded = 0;
	std::vector<unsigned char> ff(rb, 0xFF);
	for (size_t i = 0; i < I2.size(); ++i) {
		const float *r = &R[i * (size_t)d];
		if (I2[i] < 0) {
			++padded;
			bad += memcmp(r, ff.data(), rb) != 0;
		} else {
			const size_t row = with_ids ? (size_t)(I2[i] - 100) / 3 : (size_t)I2[i];
			bad += row >= n || memcmp(r, &xb[row * (size_t)d], rb) != 0;
		}
	}
	if (bad || differ || !refused || padded != 2 * nq) {
		printf("RECONSTRUCT FAIL %zu rows differ, search_and_reconstruct %s search, absent key %s, %zu padded slots (want %zu)\n", bad,
		       differ ? "differs from" : "equals", refused ? "refused" : "accepted", padded, 2 * nq);
		return 1;
	}
	printf("RECONSTRUCT OK %zu %zu\n", n, padded);
	return 0;
}

// host -> device copy rate of this box (what the ingest rates are a fraction of): 256 MiB from pinned and from pageable memory
extern "C" {
int hipHostMalloc(void **, size_t, unsigned);
int hipHostFree(void *);
int hipMalloc(void **, size_t);
int hipFree(void *);
int hipMemcpy(void *, const void *, size_t, int);
int hipDeviceSynchronize();
}
int run_linkrate() {
	const size_t bytes = (size_t)256 << 20;
	void *dev = nullptr, *pin = nullptr;
	if (hipMalloc(&dev, bytes) != 0 || hipHostMalloc(&pin, bytes, 0) != 0) {
		printf("linkrate\tFAIL allocation\n");
		return 1;
	}
	std::vector<char> page(bytes, 1);
	memset(pin, 1, bytes);
	double best[2] = {0, 0};
	for (int rep = 0; rep < 4; ++rep)
		for (int kind = 0; kind < 2; ++kind) {
			hipDeviceSynchronize();
			const auto t0 = std::chrono::steady_clock::now();
			hipMemcpy(dev, kind == 0 ? pin : (void *)page.data(), bytes, 1 /* hipMemcpyHostToDevice */);
			hipDeviceSynchronize();
			const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			best[kind] = std::max(best[kind], (double)bytes / sec / 1e9);
		}
	printf("linkjson\t{\"h2d_pinned_GBps\": %.2f, \"h2d_pageable_GBps\": %.2f, \"bytes\": %zu}\n", best[0], best[1], bytes);
	hipFree(dev);
	hipHostFree(pin);
	return 0;
}

// README.md:61 index "IDMap,HNSW32": CreateFunction with the efConstruction parameter (:127-139), chunked faiss_add with
// ids, faiss_search with SearchParametersHNSW (:691-702), then faiss_save / faiss_load (:188-240) and the same search
int run_hnsw(size_t n, int d, int threads, const char *path) {
	std::vector<float> xb(n * (size_t)d), xq(256 * (size_t)d);
	uint64_t s = 0x2545F4914F6CDD1Dull;
	auto next = [&]() {
		s ^= s << 13;
		s ^= s >> 7;
		s ^= s << 17;
		return (float)(s >> 40) * (1.0f / 16777216.0f);
	};
	for (auto &v : xb)
		v = next();
	for (auto &v : xq)
		v = next();
	std::vector<faiss::idx_t> ids(n);
	for (size_t i = 0; i < n; ++i)
		ids[i] = (faiss::idx_t)(500 + 3 * i);
	auto e = create(d, "IDMap,HNSW32", faiss::METRIC_L2);
	{ // the glue's parameter application: unwrap IDMap, dynamic_cast to IndexHNSW, set hnsw.efConstruction
		faiss::Index *ix = e->index.get();
		if (auto idmap = dynamic_cast<faiss::IndexIDMap *>(ix))
			ix = idmap->index;
		auto hnsw = dynamic_cast<faiss::IndexHNSW *>(ix);
		if (!hnsw) {
			printf("hnsw\tFAIL dynamic_cast<IndexHNSW*>\n");
			return 1;
		}
		hnsw->hnsw.efConstruction = 64;
	}
	faiss_add(*e, n, xb.data(), ids.data(), threads);
	// the graph must have been built with the value the glue assigned on the IDMap's sub-index wrapper
	const int efc = mvs_index_hnsw_get_ef_construction(e->index->handle);
	printf("hnswefc\t%s device efConstruction=%d (set 64 through IndexIDMap::index)\n", efc == 64 ? "OK" : "FAIL", efc);
	if (efc != 64)
		return 1;
	auto exact = create(d, "IDMap,Flat", faiss::METRIC_L2);
	faiss_add(*exact, n, xb.data(), ids.data(), 1);
	const size_t nq = 256, k = 10;
	auto got = faiss_search(*e, nq, xq.data(), k, nullptr, 0, 128);
	auto want = faiss_search(*exact, nq, xq.data(), k);
	size_t hits = 0;
	for (size_t q = 0; q < nq; ++q)
		for (size_t a = 0; a < k; ++a)
			for (size_t b = 0; b < k; ++b)
				hits += got[q * k + a].label == want[q * k + b].label;
	const double recall = (double)hits / (double)(nq * k);
	printf("hnsw\t%s recall@10 %.4f ntotal=%lld\n", recall >= 0.9 ? "OK" : "FAIL", recall, (long long)e->index->ntotal);
	// SaveFunction :199 / LoadFunction :234
	faiss::write_index(e->index.get(), path);
	IndexEntry loaded;
	loaded.index.reset(faiss::read_index(path));
	auto again = faiss_search(loaded, nq, xq.data(), k, nullptr, 0, 128);
	size_t same = 0;
	for (size_t i = 0; i < got.size(); ++i)
		same += got[i].label == again[i].label && got[i].distance == again[i].distance;
	printf("hnswio\t%s %zu/%zu identical rows after write_index/read_index, d=%d ntotal=%lld trained=%d\n",
	       same == got.size() ? "OK" : "FAIL", same, got.size(), loaded.index->d, (long long)loaded.index->ntotal,
	       (int)loaded.index->is_trained);
	return recall >= 0.9 && same == got.size() ? 0 : 1;
}

// "<chain>,<sub>" through the faiss:: classes: CreateFunction, train on all rows, add (with ids under IDMap), search.  Rows are
// x[i] = ((i * 2654435761 + 12345) mod 1000003) / 1000003 - 0.5 over the flat index i, column c scaled by 2 - 1.75 c / (d - 1) (computed in f64, rounded
// to f32, the product in f32); the queries are the first nq rows.  One line per query: "pretransform <index> <q> <k labels> <k
// distance words in hex>", which tests/test_pretransform_gpu.py compares with the Python host's answer for the same inputs
int run_pretransform(int d, size_t n, size_t nq, size_t k) {
	std::vector<float> xb(n * (size_t)d);
	for (size_t i = 0; i < xb.size(); ++i) {
		const double v = (double)(((uint64_t)i * 2654435761ull + 12345ull) % 1000003ull) / 1000003.0 - 0.5;
		const int c = (int)(i % (size_t)d);
		const float scale = (float)(d > 1 ? 2.0 + (0.25 - 2.0) * (double)c / (double)(d - 1) : 2.0);
		xb[i] = (float)v * scale;
	}
	struct Case {
		const char *desc;
		faiss::MetricType metric;
	} cases[] = {{"PCA8,Flat", faiss::METRIC_L2}, {"L2norm,Flat", faiss::METRIC_INNER_PRODUCT}, {"IDMap,PCAW8,IVF4,Flat", faiss::METRIC_L2}};
	for (const Case &c : cases) {
		auto e = create(d, c.desc, c.metric);
		faiss::Index *ix = e->index.get();
		const bool idmap = dynamic_cast<faiss::IndexIDMap *>(ix) != nullptr;
		if (auto m = dynamic_cast<faiss::IndexIDMap *>(ix))
			ix = m->index;
		auto *pt = dynamic_cast<faiss::IndexPreTransform *>(ix);
		if (!pt || !pt->index || pt->chain.empty() || dynamic_cast<faiss::IndexIVF *>(ix)) {
			printf("pretransform\tFAIL %s: dynamic_cast<IndexPreTransform*>\n", c.desc);
			return 1;
		}
		if (e->needs_training)
			e->index->train((faiss::idx_t)n, xb.data());
		ix->refresh_chain();
		if (!e->index->is_trained || !pt->chain[0]->is_trained || pt->chain.back()->d_out != pt->index->d) {
			printf("pretransform\tFAIL %s: not trained, or the chain does not end at the sub-index's d\n", c.desc);
			return 1;
		}
		std::vector<faiss::idx_t> ids(n);
		for (size_t i = 0; i < n; ++i)
			ids[i] = (faiss::idx_t)(7 * i + 3);
		for (size_t r0 = 0; r0 < n; r0 += STANDARD_VECTOR_SIZE) { // DataChunk-sized adds, as AddFunction makes them
			const size_t nc = std::min(STANDARD_VECTOR_SIZE, n - r0);
			if (idmap)
				e->index->add_with_ids((faiss::idx_t)nc, &xb[r0 * (size_t)d], &ids[r0]);
			else
				e->index->add((faiss::idx_t)nc, &xb[r0 * (size_t)d]);
		}
		std::vector<float> D(nq * k);
		std::vector<faiss::idx_t> I(nq * k);
		faiss::SearchParametersIVF ivf;
		ivf.nprobe = 2;
		const bool has_ivf = dynamic_cast<faiss::IndexIVF *>(pt->index) != nullptr; // (the host unwraps IndexPreTransform::index itself)
		e->index->search((faiss::idx_t)nq, xb.data(), (faiss::idx_t)k, D.data(), I.data(), has_ivf ? &ivf : nullptr);
		for (size_t q = 0; q < nq; ++q) {
			printf("pretransform %s %zu", c.desc, q);
			for (size_t j = 0; j < k; ++j)
				printf(" %lld", (long long)I[q * k + j]);
			for (size_t j = 0; j < k; ++j) {
				uint32_t w;
				memcpy(&w, &D[q * k + j], 4);
				printf(" %08x", w);
			}
			printf("\n");
		}
	}
	return 0;
}

// The binary family through the faiss:: classes (include/mi355_faiss.h "binary indexes"): an IndexBinaryFlat, wrapped by hand in an
// IndexBinaryIDMap for an "IDMap..." string (FAISS's way: its binary factory has no such prefix), filled in DataChunk-sized adds, then
// search, range_search and a file round trip, each checked against a plain popcount loop
int run_binary(size_t n, int d, size_t nq, const char *desc) {
	const size_t cs = (size_t)d / 8, k = 10;
	std::vector<uint8_t> xb(n * cs), xq(nq * cs);
	uint64_t s = 0x9E3779B97F4A7C15ull;
	auto next = [&]() {
		s ^= s << 13;
		s ^= s >> 7;
		s ^= s << 17;
		return (uint8_t)(s >> 32);
	};
	for (auto &v : xb)
		v = next();
	for (auto &v : xq)
		v = next();
	for (size_t q = 0; q < nq && q < n; q += 3) // exact duplicates: hits of radius 1
		memcpy(&xb[(n - 1 - q) * cs], &xq[q * cs], cs);
	const bool with_ids = !strncmp(desc, "IDMap", 5);
	std::vector<faiss::idx_t> ids(n);
	for (size_t i = 0; i < n; ++i)
		ids[i] = with_ids ? (faiss::idx_t)(7 * i + 3) : (faiss::idx_t)i;
	std::unique_ptr<faiss::IndexBinary> flat, index;
	if (with_ids) {
		flat.reset(new faiss::IndexBinaryFlat(d));
		index.reset(new faiss::IndexBinaryIDMap(flat.get()));
	} else {
		index.reset(faiss::index_binary_factory(d, desc));
	}
	for (size_t i0 = 0; i0 < n; i0 += 2048) {
		const size_t nb = std::min<size_t>(2048, n - i0);
		if (with_ids)
			index->add_with_ids((faiss::idx_t)nb, &xb[i0 * cs], &ids[i0]);
		else
			index->add((faiss::idx_t)nb, &xb[i0 * cs]);
	}
	auto ham = [&](size_t q, size_t r) {
		int h = 0;
		for (size_t j = 0; j < cs; ++j)
			h += __builtin_popcount((unsigned)(xq[q * cs + j] ^ xb[r * cs + j]));
		return h;
	};
	const int radius = d / 2 - d / 8;
	size_t bad_search = 0, bad_range = 0, bad_file = 0, hits = 0;
	auto check_search = [&](const faiss::IndexBinary &ix, size_t &bad) {
		std::vector<int32_t> D(nq * k);
		std::vector<faiss::idx_t> I(nq * k);
		ix.search((faiss::idx_t)nq, xq.data(), (faiss::idx_t)k, D.data(), I.data());
		std::vector<std::pair<int, size_t>> all(n);
		for (size_t q = 0; q < nq; ++q) {
			for (size_t r = 0; r < n; ++r)
				all[r] = {ham(q, r), r};
			std::sort(all.begin(), all.end());
			for (size_t j = 0; j < k; ++j) {
				const bool pad = j >= n;
				const int32_t wd = pad ? 2147483647 : all[j].first;
				const faiss::idx_t wi = pad ? -1 : ids[all[j].second];
				bad += D[q * k + j] != wd || I[q * k + j] != wi;
			}
		}
	};
	check_search(*index, bad_search);
	{
		faiss::RangeSearchResult res(nq);
		index->range_search((faiss::idx_t)nq, xq.data(), radius, &res);
		size_t pos = 0;
		for (size_t q = 0; q < nq; ++q) {
			bad_range += res.lims[q] != pos;
			for (size_t r = 0; r < n; ++r) {
				const int h = ham(q, r);
				if (h >= radius)
					continue;
				if (pos >= res.lims[nq] || res.labels[pos] != ids[r] || res.distances[pos] != (float)h)
					++bad_range;
				++pos;
			}
		}
		bad_range += res.lims[nq] != pos;
		hits = pos;
	}
	{
		char fname[64];
		snprintf(fname, sizeof fname, "/tmp/boundary_driver_binary_%d.idx", (int)getpid());
		faiss::write_index_binary(index.get(), fname);
		std::unique_ptr<faiss::IndexBinary> back(faiss::read_index_binary(fname));
		remove(fname);
		bad_file += back->ntotal != index->ntotal || back->d != d || (dynamic_cast<faiss::IndexBinaryIDMap *>(back.get()) != nullptr) != with_ids;
		check_search(*back, bad_file);
		std::vector<uint8_t> row(cs);
		back->reconstruct(ids[n / 2], row.data());
		bad_file += memcmp(row.data(), &xb[(n / 2) * cs], cs) != 0;
	}
	if ((size_t)index->ntotal != n || index->code_size != (int)cs || bad_search || bad_range || bad_file) {
		printf("BINARY FAIL ntotal %lld (want %zu), %zu search entries, %zu range entries, %zu entries after the file round trip differ\n",
		       (long long)index->ntotal, n, bad_search, bad_range, bad_file);
		return 1;
	}
	printf("BINARY OK %s n %zu d %d nq %zu k %zu radius %d hits %zu\n", desc, n, d, nq, k, radius, hits);
	return 0;
}

} // namespace

int main(int argc, char **argv) {
	try {
		if (argc >= 4 && !strcmp(argv[1], "golden"))
			return run_golden(argv[2], argv[3]);
		if (argc >= 5 && !strcmp(argv[1], "ingest"))
			return run_ingest((size_t)atoll(argv[2]), atoi(argv[3]), atoi(argv[4]), argc >= 6 ? argv[5] : "IDMap,Flat");
		if (argc >= 4 && !strcmp(argv[1], "ivfpq"))
			return run_ivfpq((size_t)atoll(argv[2]), atoi(argv[3]));
		if (argc >= 2 && !strcmp(argv[1], "linkrate"))
			return run_linkrate();
		if (argc >= 6 && !strcmp(argv[1], "range"))
			return run_range((size_t)atoll(argv[2]), atoi(argv[3]), (size_t)atoll(argv[4]), argv[5]);
		if (argc >= 6 && !strcmp(argv[1], "remove"))
			return run_remove((size_t)atoll(argv[2]), atoi(argv[3]), (size_t)atoll(argv[4]), argv[5]);
		if (argc >= 6 && !strcmp(argv[1], "selectors"))
			return run_selectors((size_t)atoll(argv[2]), atoi(argv[3]), (size_t)atoll(argv[4]), argv[5]);
		if (argc >= 6 && !strcmp(argv[1], "merge"))
			return run_merge((size_t)atoll(argv[2]), atoi(argv[3]), (size_t)atoll(argv[4]), argv[5]);
		if (argc >= 6 && !strcmp(argv[1], "reconstruct"))
			return run_reconstruct((size_t)atoll(argv[2]), atoi(argv[3]), (size_t)atoll(argv[4]), argv[5]);
		if (argc >= 6 && !strcmp(argv[1], "pretransform"))
			return run_pretransform(atoi(argv[2]), (size_t)atoll(argv[3]), (size_t)atoll(argv[4]), (size_t)atoll(argv[5]));
		if (argc >= 6 && !strcmp(argv[1], "binary"))
			return run_binary((size_t)atoll(argv[2]), atoi(argv[3]), (size_t)atoll(argv[4]), argv[5]);
		if (argc >= 6 && !strcmp(argv[1], "hnsw"))
			return run_hnsw((size_t)atoll(argv[2]), atoi(argv[3]), atoi(argv[4]), argv[5]);
	} catch (const std::exception &e) {
		fprintf(stderr, "fatal: %s\n", e.what());
		return 3;
	}
	fprintf(stderr, "usage: boundary_driver golden <training.csv> <queries.csv> | ingest <n> <d> <threads> [index] | linkrate | "
	                "hnsw <n> <d> <threads> <index file> | ivfpq <n> <d> | range <rows> <d> <nq> <index> | remove <rows> <d> <nq> <index> | "
	                "selectors <rows> <d> <nq> <index> | merge <rows> <d> <nq> <index> | reconstruct <rows> <d> <nq> <index> | pretransform <d> <n> <nq> <k> | binary <rows> <d bits> <nq> <index>\n");
	return 2;
}
