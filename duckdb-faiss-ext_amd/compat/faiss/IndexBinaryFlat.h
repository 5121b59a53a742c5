// compat/faiss/IndexBinaryFlat.h -- faiss::IndexBinaryFlat: exhaustive Hamming search on the device (csrc/binary.hip)
#pragma once
#include "IndexBinary.h"
namespace faiss {
struct IndexBinaryFlat : IndexBinary {
	IndexBinaryFlat() = default; // (a wrapper for an existing handle: IndexBinary::wrap)
	explicit IndexBinaryFlat(idx_t d);
};
} // namespace faiss
