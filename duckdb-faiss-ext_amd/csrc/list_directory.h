// csrc/list_directory.h -- the host directory of an index with inverted lists (IVF<n>,Flat: csrc/ivf.hip; the coded kinds: csrc/coded_lists.hip;
// DESIGN.md 3.16).  Plain C++, no HIP: a stand-alone program compiles it (tests/test_list_directory_cpu.py builds one with the sanitizers).
// Rows are named by ARRIVAL POSITION, the row number of the kind's append-only store.  The directory says which list a position belongs to
// and which id it was stored under; every view of the lists (the list-sorted store, an image, a removal plan) is derived from it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mvs {

struct IvfRemovePlan; // csrc/remove_plan.h

struct ListDirectory {
	int64_t nlist;
	std::vector<int32_t> assign; // [rows] list of the row at an arrival position; -1: in no list (FAISS never stored it)
	std::vector<int64_t> ids;    // [rows] its stored id
	explicit ListDirectory(int64_t nlist_) : nlist(nlist_) {
	}
	int64_t rows() const {
		return (int64_t)ids.size();
	}
	void reserve(int64_t n) {
		assign.reserve((size_t)n), ids.reserve((size_t)n);
	}
	// n rows arrive with the quantiser's k = 1 labels; their ids are ids_in[i], or first_id + i without ids_in.  A label outside
	// [0, nlist) becomes -1.  The only such label a quantiser returns is -1 (no finite nearest centroid), so the clamp is the single rule
	// for every kind and changes nothing reachable
	void append(int64_t n, const int64_t *labels, const int64_t *ids_in, int64_t first_id) {
		for (int64_t i = 0; i < n; i++) {
			const int64_t l = labels[i];
			assign.push_back(l >= 0 && l < nlist ? (int32_t)l : -1);
			ids.push_back(ids_in ? ids_in[i] : first_id + i);
		}
	}
	// The counting sort: arrival positions grouped by list, arrival order inside a list (ArrayInvertedLists semantics).  List l holds the
	// list-sorted positions [off[l], off[l + 1]); perm[p] is the arrival position at list-sorted position p, ids[perm[p]] its stored id
	struct Groups {
		std::vector<int64_t> off;  // [nlist + 1]
		std::vector<int32_t> perm; // [off[nlist]]
	};
	static Groups group(int64_t nlist, const std::vector<int32_t> &assign) {
		Groups g;
		g.off.assign((size_t)nlist + 1, 0);
		for (int32_t l : assign)
			if (l >= 0)
				g.off[(size_t)l + 1]++;
		for (int64_t l = 0; l < nlist; l++)
			g.off[(size_t)l + 1] += g.off[(size_t)l];
		g.perm.resize((size_t)g.off[(size_t)nlist]);
		std::vector<int64_t> cursor(g.off.begin(), g.off.end() - 1);
		for (size_t i = 0; i < assign.size(); i++)
			if (assign[i] >= 0)
				g.perm[(size_t)cursor[(size_t)assign[i]]++] = (int32_t)i;
		return g;
	}
	Groups group() const {
		return group(nlist, assign);
	}
	std::vector<int64_t> sorted_ids(const Groups &g) const {
		std::vector<int64_t> sid(g.perm.size());
		for (size_t p = 0; p < sid.size(); p++)
			sid[p] = ids[(size_t)g.perm[p]];
		return sid;
	}
	// an ArrayInvertedLists image: per list the stored ids and the arrival positions of its rows (the kind copies the row bytes from there)
	void to_lists(std::vector<std::vector<int64_t>> &list_ids, std::vector<std::vector<int32_t>> &list_pos) const {
		const Groups g = group();
		list_ids.assign((size_t)nlist, {});
		list_pos.assign((size_t)nlist, {});
		for (int64_t l = 0; l < nlist; l++) {
			list_pos[(size_t)l].assign(g.perm.begin() + g.off[(size_t)l], g.perm.begin() + g.off[(size_t)l + 1]);
			for (int32_t i : list_pos[(size_t)l])
				list_ids[(size_t)l].push_back(ids[(size_t)i]);
		}
	}
	// ... and back: the rows of an image enter list-major, which keeps the arrival order inside every list.  Returns the row count
	int64_t adopt_image(const std::vector<std::vector<int64_t>> &list_ids) {
		assign.clear(), ids.clear();
		for (int64_t l = 0; l < nlist; l++)
			for (int64_t id : list_ids[(size_t)l]) {
				assign.push_back((int32_t)l);
				ids.push_back(id);
			}
		return rows();
	}
	// merge_from (include/mi355_faiss.h "merge_from and copy_subset_to"): the rows of `o` arrive behind this directory's in o's arrival order,
	// each in its list (or in none) with its stored id + add_id -- which puts them behind this directory's entries in every list, in o's
	// list order.  Only the positions pos[0 .. npos) of `o` with `pos` given (copy_subset_to)
	void append_from(const ListDirectory &o, int64_t add_id, const std::vector<int64_t> *pos = nullptr) {
		const size_t n = pos ? pos->size() : o.ids.size();
		assign.reserve(assign.size() + n), ids.reserve(ids.size() + n); // (the only step that can fail: nothing has changed yet)
		for (size_t i = 0; i < n; i++) {
			const size_t p = pos ? (size_t)(*pos)[i] : i;
			assign.push_back(o.assign[p]);
			ids.push_back(o.ids[p] + add_id);
		}
	}
	// copy_subset_to: the arrival positions of the LISTED rows a subset type selects, ascending (so they stay in list order inside every
	// list).  0: stored id in [a1, a2); 1: id % a1 == a2 with C++'s % (the caller refuses a1 <= 0); 2: entries [i1, i2) of every list by the
	// running sums of FAISS's InvertedLists::copy_subset_to (UNVERIFIED, restated from memory: include/mi355_faiss.h), ntotal as the caller
	// counts it.  Another type selects nothing (the caller refuses it)
	std::vector<int64_t> subset(int type, int64_t a1, int64_t a2, int64_t ntotal) const {
		std::vector<int64_t> pos;
		if (type == 0 || type == 1) {
			for (size_t i = 0; i < ids.size(); i++)
				if (assign[i] >= 0 && (type == 0 ? (ids[i] >= a1 && ids[i] < a2) : (a1 > 0 && ids[i] % a1 == a2)))
					pos.push_back((int64_t)i);
		} else if (type == 2 && ntotal > 0) {
			const Groups g = group();
			int64_t accu_n = 0, accu_a1 = 0, accu_a2 = 0;
			for (int64_t l = 0; l < nlist; l++) {
				const int64_t n = g.off[(size_t)l + 1] - g.off[(size_t)l];
				const int64_t next_n = accu_n + n;
				const int64_t i1 = (int64_t)((__int128)next_n * a1 / ntotal) - accu_a1, i2 = (int64_t)((__int128)next_n * a2 / ntotal) - accu_a2;
				for (int64_t i = i1 < 0 ? 0 : i1; i < i2 && i < n; i++)
					pos.push_back((int64_t)g.perm[(size_t)(g.off[(size_t)l] + i)]);
				accu_n = next_n, accu_a1 += i1, accu_a2 += i2;
			}
			std::sort(pos.begin(), pos.end());
		}
		return pos;
	}
	void adopt(IvfRemovePlan &&plan); // the directory a removal leaves (csrc/remove_plan.h), once the caller's store is gathered by plan.perm
};

} // namespace mvs
