// csrc/remove_plan.h -- the host plan of remove_ids (include/mi355_faiss.h "remove_ids").  Plain C++, no HIP: a stand-alone
// program compiles it (tests/test_remove_cabi_cpu.py builds one with the sanitizers), as csrc/flat_collect.h under MVS_COLLECT_PLAN_ONLY.
//
//   RemoveSelector     membership on the host: a bitmap lookup; a batch as a dense bit array over [min, max], or -- a wide span -- sorted
//                      once and bisected
//   ivf_remove_plan    the IVF kinds.  From the keep flags in arrival order, assign_h and ids_h: every list runs FAISS's swap-from-the-end
//                      loop on its own, over ListDirectory's grouping (csrc/list_directory.h); the new arrival order is list-major (what
//                      adopt_image produces, so build_lists sees nothing new); `perm` gathers the arrival-order store; ids are renumbered
//                      under IDMap.  ListDirectory::adopt takes the plan over
//   remove_renumber    under IDMap: new stored id of s = s - #{removed r < s}
#pragma once
#include "list_directory.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mvs {

struct RemoveSelector {
	static constexpr int64_t DENSE_BYTES = (int64_t)64 << 20; // a batch whose ids span at most this many bytes of bits is looked up densely
	int kind = 0; // 1: bitmap, 2: batch (MVS_SEL_BITMAP / MVS_SEL_BATCH)
	const uint8_t *bitmap = nullptr;
	int64_t nbytes = 0;
	std::vector<int64_t> sorted;
	std::vector<uint8_t> dense; // batch: bit (id - lo) is set, when the span allows it (10 M lookups by bisection were 215-340 ms)
	int64_t lo = 0, hi = -1;
	RemoveSelector(int kind_, const void *data, int64_t n) : kind(kind_) {
		if (kind == 1) {
			bitmap = (const uint8_t *)data;
			nbytes = n;
		} else if (kind == 2 && n > 0) {
			const int64_t *ids = (const int64_t *)data;
			lo = *std::min_element(ids, ids + n);
			hi = *std::max_element(ids, ids + n);
			if ((uint64_t)hi - (uint64_t)lo < (uint64_t)DENSE_BYTES * 8) {
				dense.assign((size_t)(((uint64_t)hi - (uint64_t)lo) / 8 + 1), 0);
				for (int64_t i = 0; i < n; ++i) {
					const uint64_t u = (uint64_t)ids[i] - (uint64_t)lo;
					dense[(size_t)(u >> 3)] |= (uint8_t)(1u << (u & 7));
				}
			} else {
				sorted.assign(ids, ids + n);
				std::sort(sorted.begin(), sorted.end());
			}
		}
	}
	// bitmap: bit `id` is set; a negative id or one beyond the bitmap is no member.  Batch: id occurs in the list
	bool member(int64_t id) const {
		if (kind == 1) {
			const uint64_t u = (uint64_t)id;
			if ((u >> 3) >= (uint64_t)nbytes)
				return false;
			return (bitmap[u >> 3] >> (u & 7)) & 1;
		}
		if (!dense.empty()) {
			if (id < lo || id > hi)
				return false;
			const uint64_t u = (uint64_t)id - (uint64_t)lo;
			return (dense[(size_t)(u >> 3)] >> (u & 7)) & 1;
		}
		return std::binary_search(sorted.begin(), sorted.end(), id);
	}
};

// true iff ids holds every value of 0 .. n-1 exactly once (n = ids.size()): what an IVF index under IDMap stores unless a foreign file built it
inline bool remove_ids_are_permutation(const std::vector<int64_t> &ids) {
	const int64_t n = (int64_t)ids.size();
	std::vector<uint8_t> seen((size_t)n, 0);
	for (int64_t v : ids) {
		if (v < 0 || v >= n || seen[(size_t)v])
			return false;
		seen[(size_t)v] = 1;
	}
	return true;
}

// renum[s] = s - #{r < s : !keep[r]} (meaningful for survivors only)
inline std::vector<int64_t> remove_renumber(const std::vector<uint8_t> &keep_by_id) {
	std::vector<int64_t> renum(keep_by_id.size());
	int64_t kept = 0;
	for (size_t s = 0; s < keep_by_id.size(); ++s) {
		renum[s] = kept;
		kept += keep_by_id[s] ? 1 : 0;
	}
	return renum;
}

struct IvfRemovePlan {
	std::vector<int32_t> perm;   // [nkeep] new arrival position -> old arrival position
	std::vector<int32_t> assign; // [nkeep] the new assign_h
	std::vector<int64_t> ids;    // [nkeep] the new ids_h
	int64_t removed = 0;
};

// keep[i]: the row at arrival position i stays.  A row without a list (assign < 0: it is in no inverted list, FAISS never stored it) is
// bookkeeping only: a survivor keeps its place behind the lists.  renum (or null): new stored id by old stored id
inline void ivf_remove_plan(int64_t nlist, const std::vector<int32_t> &assign_h, const std::vector<int64_t> &ids_h, const std::vector<uint8_t> &keep,
                            const std::vector<int64_t> *renum, IvfRemovePlan &out) {
	const int64_t n = (int64_t)assign_h.size();
	ListDirectory::Groups g = ListDirectory::group(nlist, assign_h);
	const std::vector<int64_t> &off = g.off;
	std::vector<int32_t> &pos = g.perm; // arrival positions grouped by list, arrival order inside a list: the swap loops work in place
	out.perm.clear(), out.assign.clear(), out.ids.clear();
	out.perm.reserve((size_t)n), out.assign.reserve((size_t)n);
	out.removed = 0;
	for (int64_t l = 0; l < nlist; ++l) {
		int32_t *p = pos.data() + off[(size_t)l];
		// FAISS's loop over one list (IndexIVF::remove_ids -> InvertedLists): j does not advance after a swap
		int64_t len = off[(size_t)l + 1] - off[(size_t)l], j = 0;
		while (j < len) {
			if (!keep[(size_t)p[j]]) {
				--len;
				p[j] = p[len];
			} else
				++j;
		}
		out.removed += off[(size_t)l + 1] - off[(size_t)l] - len;
		for (j = 0; j < len; ++j) {
			out.perm.push_back(p[j]);
			out.assign.push_back((int32_t)l);
		}
	}
	for (int64_t i = 0; i < n; ++i)
		if (assign_h[(size_t)i] < 0) {
			if (!keep[(size_t)i]) {
				++out.removed;
				continue;
			}
			out.perm.push_back((int32_t)i);
			out.assign.push_back(-1);
		}
	out.ids.resize(out.perm.size());
	for (size_t i = 0; i < out.perm.size(); ++i) {
		const int64_t id = ids_h[(size_t)out.perm[i]];
		out.ids[i] = renum ? (*renum)[(size_t)id] : id;
	}
}

inline void ListDirectory::adopt(IvfRemovePlan &&plan) {
	assign = std::move(plan.assign);
	ids = std::move(plan.ids);
}

} // namespace mvs
