#pragma once
#include "Index.h"
#include "IndexBinary.h"
namespace faiss {
void write_index(const Index *idx, const char *fname); // src/faiss_extension.cpp:199
Index *read_index(const char *fname, int io_flags = 0); // :234
void write_index_binary(const IndexBinary *idx, const char *fname);
IndexBinary *read_index_binary(const char *fname, int io_flags = 0);
} // namespace faiss
