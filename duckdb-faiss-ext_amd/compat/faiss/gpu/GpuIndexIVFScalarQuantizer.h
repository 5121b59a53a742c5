// compat/faiss/gpu/GpuIndexIVFScalarQuantizer.h -- faiss::gpu::GpuIndexIVFScalarQuantizer(provider, dims, nlist, qtype, metric,
// encodeResidual) over mvs_gpu_index_ivfsq_new (include/mi355_faiss.h "fp16 scalar-quantised inverted lists"): QT_8bit is the index
// index_factory("IVF<n>,SQ8") gives, QT_fp16 the fp16 lists, which no factory string reaches.  Every other qtype, encodeResidual = false,
// a metric beyond L2 / inner product and dims > 2048 throw "This index type is not implemented on the MI355X path yet: ..."
#pragma once
#include "GpuIndexIVF.h"
#include "StandardGpuResources.h"
namespace faiss {
namespace gpu {
struct GpuIndexIVFScalarQuantizer : GpuIndexIVF {
	faiss::ScalarQuantizer sq;
	bool by_residual = true;
	size_t nlist = 0;
	GpuIndexIVFScalarQuantizer(GpuResourcesProvider *, int dims, idx_t nlist_, faiss::ScalarQuantizer::QuantizerType qtype,
	                           faiss::MetricType metric = faiss::METRIC_L2, bool encodeResidual = true) {
		if (mvs_gpu_index_ivfsq_new(&handle, dims, (int64_t)nlist_, (int)qtype, (int)metric, encodeResidual ? 1 : 0))
			throw_last_error();
		refresh();
		nlist = (size_t)nlist_;
		sq.qtype = qtype;
		sq.d = (size_t)dims;
		sq.bits = qtype == faiss::ScalarQuantizer::QT_fp16 ? 16 : 8;
		sq.code_size = sq.d * sq.bits / 8;
	}
};
} // namespace gpu
} // namespace faiss
