// compat/faiss/IndexIDMap.h -- the glue reads and re-assigns IndexIDMap::index (src/faiss_extension.cpp:127-130,671-674)
#pragma once
#include "Index.h"
#include "IndexBinary.h"
namespace faiss {
struct IndexIDMap : Index {
	Index *index = nullptr; // borrowed view of the sub-index (owned by the device object)
	bool own_fields = false;
	~IndexIDMap() override;
	void before_add() override; // "IDMap,HNSW32" + map{'efConstruction':..}: the glue sets it on `index`, adds on the wrapper
	void before_search() const override;
	void refresh_chain() override;
};
// faiss::IndexBinaryIDMap: the FAISS way to external ids on a binary index (its binary factory has no IDMap prefix) -- wrap an EMPTY
// IndexBinaryFlat by hand.  The wrapper takes the rows and the ids; `index` stays a view of the wrapped index (labels are row numbers)
struct IndexBinaryIDMap : IndexBinary {
	IndexBinary *index = nullptr;
	bool own_fields = false; // FAISS's member: the wrapped object is deleted with the wrapper
	IndexBinaryIDMap() = default;
	explicit IndexBinaryIDMap(IndexBinary *index);
	~IndexBinaryIDMap() override;
	void refresh() override;

private:
	IndexBinary *given_ = nullptr; // the object the constructor was handed
};
} // namespace faiss
