// compat/faiss/impl/IDSelector.h -- IDSelectorBitmap (src/faiss_extension.cpp:959), IDSelectorBatch (:1008).
// The selector memory stays owned by the glue (mask_tmp / a local vector) and only has to outlive the search call;
// the device path copies it to HBM per call (csrc/index.hip SelectorHolder).
// The other classes of faiss/impl/IDSelector.h -- Range, Array, All, Not, And, Or, XOr -- which the glue never builds: they borrow their
// children / arrays as FAISS's do, and the adaptor flattens a tree of them to one MVS_SEL_PROGRAM (include/mi355_faiss.h "selector programs").
#pragma once
#include "../MetricType.h"

#include <cstddef>
#include <cstdint>
#include <vector>
namespace faiss {
struct IDSelector {
	virtual bool is_member(idx_t id) const = 0;
	virtual ~IDSelector() {
	}
};
struct IDSelectorBitmap : IDSelector {
	size_t n;
	const uint8_t *bitmap;
	IDSelectorBitmap(size_t n_, const uint8_t *bitmap_) : n(n_), bitmap(bitmap_) {
	}
	bool is_member(idx_t ii) const final {
		uint64_t i = (uint64_t)ii;
		if ((i >> 3) >= n)
			return false;
		return (bitmap[i >> 3] >> (i & 7)) & 1;
	}
};
struct IDSelectorBatch : IDSelector {
	std::vector<idx_t> ids; // FAISS keeps a bloom filter + hash set; membership is what matters
	IDSelectorBatch(size_t n, const idx_t *indices) : ids(indices, indices + n) {
	}
	bool is_member(idx_t id) const final {
		for (idx_t v : ids)
			if (v == id)
				return true;
		return false;
	}
};
struct IDSelectorRange : IDSelector {
	idx_t imin, imax;
	bool assume_sorted; // (FAISS: the ids of a list are sorted, so a list is cut by bisection -- no meaning on this path, ignored)
	IDSelectorRange(idx_t imin_, idx_t imax_, bool assume_sorted_ = false) : imin(imin_), imax(imax_), assume_sorted(assume_sorted_) {
	}
	bool is_member(idx_t id) const final {
		return id >= imin && id < imax;
	}
};
struct IDSelectorArray : IDSelector { // the caller's array, borrowed
	size_t n;
	const idx_t *ids;
	IDSelectorArray(size_t n_, const idx_t *ids_) : n(n_), ids(ids_) {
	}
	bool is_member(idx_t id) const final {
		for (size_t i = 0; i < n; ++i)
			if (ids[i] == id)
				return true;
		return false;
	}
};
struct IDSelectorAll : IDSelector {
	bool is_member(idx_t) const final {
		return true;
	}
};
struct IDSelectorNot : IDSelector {
	const IDSelector *sel;
	explicit IDSelectorNot(const IDSelector *sel_) : sel(sel_) {
	}
	bool is_member(idx_t id) const final {
		return !sel->is_member(id);
	}
};
struct IDSelectorAnd : IDSelector {
	const IDSelector *lhs, *rhs;
	IDSelectorAnd(const IDSelector *lhs_, const IDSelector *rhs_) : lhs(lhs_), rhs(rhs_) {
	}
	bool is_member(idx_t id) const final {
		return lhs->is_member(id) && rhs->is_member(id);
	}
};
struct IDSelectorOr : IDSelector {
	const IDSelector *lhs, *rhs;
	IDSelectorOr(const IDSelector *lhs_, const IDSelector *rhs_) : lhs(lhs_), rhs(rhs_) {
	}
	bool is_member(idx_t id) const final {
		return lhs->is_member(id) || rhs->is_member(id);
	}
};
struct IDSelectorXOr : IDSelector {
	const IDSelector *lhs, *rhs;
	IDSelectorXOr(const IDSelector *lhs_, const IDSelector *rhs_) : lhs(lhs_), rhs(rhs_) {
	}
	bool is_member(idx_t id) const final {
		return lhs->is_member(id) != rhs->is_member(id);
	}
};
} // namespace faiss
