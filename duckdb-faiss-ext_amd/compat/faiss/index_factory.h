#pragma once
#include "Index.h"
#include "IndexBinary.h"
namespace faiss {
// src/faiss_extension.cpp:154-155
Index *index_factory(int d, const char *description, MetricType metric = METRIC_L2);
// "BFlat", "IDMap,BFlat", "IDMap2,BFlat"; d in bits (include/mi355_faiss.h "binary indexes")
IndexBinary *index_binary_factory(int d, const char *description);
} // namespace faiss
