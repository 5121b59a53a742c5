// compat/faiss/IndexIVFPQFastScan.h -- faiss::IndexIVFPQFastScan(quantizer, d, nlist, M, nbits, metric) over mvs_index_ivfpqfs_new
// (include/mi355_faiss.h "inverted lists of 4-bit product-quantised residuals"): 4-bit codes in inverted lists, scanned on the int8 matrix
// pipe, which no factory string reaches.  The device index owns its Flat quantiser: the one passed in gives the metric's type and is not
// adopted.  nbits != 4, an odd M, M > 128 and a metric beyond L2 / inner product throw "This index type is not implemented on the MI355X
// path yet: ..."
#pragma once
#include "IndexIVF.h"
namespace faiss {
struct IndexIVFPQFastScan : IndexIVF {
	ProductQuantizer pq;
	bool by_residual = true;
	IndexIVFPQFastScan(Index *, size_t d_, size_t nlist_, size_t M, size_t nbits = 4, MetricType metric = METRIC_L2) {
		if (mvs_index_ivfpqfs_new(&handle, (int)d_, (int64_t)nlist_, (int)M, (int)nbits, (int)metric))
			throw_last_error();
		refresh();
		nlist = nlist_;
		pq.d = d_, pq.M = M, pq.nbits = nbits, pq.dsub = d_ / M, pq.ksub = (size_t)1 << nbits, pq.code_size = (M * nbits + 7) / 8;
	}
};
} // namespace faiss
