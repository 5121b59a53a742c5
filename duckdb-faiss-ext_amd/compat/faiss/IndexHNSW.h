// compat/faiss/IndexHNSW.h -- IndexHNSW::hnsw.efConstruction (src/faiss_extension.cpp:138), SearchParametersHNSW
// (:693-699); IndexPQ / SearchParametersPQ (:704-706): the cast matches the device's PQ<M> index (MVS_KIND_PQ).
#pragma once
#include "Index.h"
#include "IndexIVF.h" // (ScalarQuantizer / IndexScalarQuantizer)
#include "impl/HNSW.h"
namespace faiss {
struct SearchParametersHNSW : SearchParameters {
	int efSearch = 16;
	bool check_relative_distance = true;
	bool bounded_queue = true;
};
struct IndexHNSW : Index {
	HNSW hnsw;
	Index *storage = nullptr;
	void before_add() override; // pushes hnsw.efConstruction to the device index
};
struct IndexHNSWFlat : IndexHNSW {};
// faiss::IndexHNSWSQ over the device's HNSW<M>,SQ8 index (MVS_KIND_HNSWSQ): an IndexHNSW -- the glue's casts at :133 and :691 reach it --;
// `storage` is an IndexScalarQuantizer VIEW of the same device index (d, ntotal, is_trained and the quantizer's geometry), owned here
struct IndexHNSWSQ : IndexHNSW {
	~IndexHNSWSQ() override;
};
struct SearchParametersPQ : SearchParameters { // (the glue builds one and sets nothing on it, :706)
	int search_type = 0; // IndexPQ::ST_PQ
	int polysemous_ht = 0;
};
// faiss::IndexPQ over the device index: pq.M / pq.nbits / pq.dsub / pq.ksub as FAISS's ProductQuantizer names them
struct IndexPQ : Index {
	struct {
		size_t d = 0, M = 0, nbits = 8, dsub = 0, ksub = 256, code_size = 0;
	} pq;
};
} // namespace faiss
