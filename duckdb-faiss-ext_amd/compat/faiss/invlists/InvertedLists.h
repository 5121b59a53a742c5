// compat/faiss/invlists/InvertedLists.h -- the subset types of faiss::IndexIVF::copy_subset_to (include/mi355_faiss.h "merge_from and
// copy_subset_to").  The lists themselves live on the device behind the C ABI: no InvertedLists object is exposed
#pragma once
namespace faiss {
struct InvertedLists {
	enum subset_type_t : int {
		SUBSET_TYPE_ID_RANGE = 0,      // stored id in [a1, a2)
		SUBSET_TYPE_ID_MOD = 1,        // id % a1 == a2
		// a range of every list's entries by FAISS's running sums.  Consecutive (a1, a2) that tile [0, ntotal) miss no row, but take a row
		// twice where a part meets a list whose rounded range is inverted (ntotal 7, cuts 2 | 3 | 4): include/mi355_faiss.h has the rule
		SUBSET_TYPE_ELEMENT_RANGE = 2,
		SUBSET_TYPE_INVLIST_FRACTION = 3, // not implemented on the MI355X path: "subset type not implemented"
		SUBSET_TYPE_INVLIST = 4,          // (the same)
	};
};
} // namespace faiss
