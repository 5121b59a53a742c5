"""ListDirectory::append_from and ListDirectory::subset (csrc/list_directory.h), the host side of merge_from and copy_subset_to: a stand-alone
C++ program, built here with AddressSanitizer and UBSan and run as a process of its own (nothing is loaded into Python).  Both functions
are checked against loops written out in the program.  Shapes: nlist 1, 3 and 7; 0, 1 and 40 rows on either side; labels that include -1;
empty lists; negative ids for the modulo; duplicated ids; group() of the merged directory against the concatenation of the two sides'
lists; the element-range type's formula as include/mi355_faiss.h states it, and what it gives for consecutive (a1, a2) ranges that tile [0, ntotal):
no listed row is missed, and every listed row is selected exactly once unless a part met a list whose rounded range is inverted (i1 > i2)
-- which the formula does not exclude for lists much smaller than a part."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "duckdb-faiss-ext_amd", "csrc")

PROGRAM = r"""
#include "list_directory.h"
#include <cstdio>
#include <cstdlib>
using namespace mvs;
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return rng_state;
}
enum Labels { MIXED, ONE_LIST, SPARSE };
static ListDirectory make_dir(int64_t nlist, int64_t n, Labels lk, bool negative_ids) {
	ListDirectory d(nlist);
	for (int64_t i = 0; i < n; i++) {
		int64_t l;
		if (lk == ONE_LIST)
			l = nlist - 1;
		else if (lk == SPARSE)
			l = (rnd() % 3 == 0) ? -1 : (int64_t)(rnd() % (uint64_t)((nlist + 1) / 2)) * 2 % nlist; // odd lists stay empty, a third of the rows in no list
		else
			l = (int64_t)(rnd() % (uint64_t)(nlist + 1)) - 1;
		const int64_t id = negative_ids ? (int64_t)(rnd() % 23) - 11 : (int64_t)(rnd() % 1000); // (duplicates in both)
		d.append(1, &l, &id, 0);
	}
	return d;
}
// the entries of list l in list order, written out: (id, arrival position)
static std::vector<std::pair<int64_t, int64_t>> list_entries(const ListDirectory &d, int64_t l) {
	std::vector<std::pair<int64_t, int64_t>> e;
	for (int64_t i = 0; i < d.rows(); i++)
		if (d.assign[(size_t)i] == l)
			e.push_back({d.ids[(size_t)i], i});
	return e;
}

static void check_append(const ListDirectory &a, const ListDirectory &b, int64_t add_id, const char *what) {
	ListDirectory m = a;
	m.append_from(b, add_id);
	CHECK(m.rows() == a.rows() + b.rows() && m.nlist == a.nlist, "%s: rows", what);
	for (int64_t i = 0; i < m.rows(); i++) { // arrival order: a's rows, then b's, each with its list and b's with id + add_id
		const bool from_a = i < a.rows();
		const int64_t j = from_a ? i : i - a.rows();
		CHECK(m.assign[(size_t)i] == (from_a ? a : b).assign[(size_t)j], "%s: assign of row %lld", what, (long long)i);
		CHECK(m.ids[(size_t)i] == (from_a ? a.ids[(size_t)j] : b.ids[(size_t)j] + add_id), "%s: id of row %lld", what, (long long)i);
	}
	// every list: a's entries, then b's in b's list order -- through group(), the view the index derives
	const ListDirectory::Groups g = m.group();
	const std::vector<int64_t> sid = m.sorted_ids(g);
	for (int64_t l = 0; l < m.nlist; l++) {
		std::vector<std::pair<int64_t, int64_t>> want = list_entries(a, l);
		for (auto e : list_entries(b, l))
			want.push_back({e.first + add_id, e.second + a.rows()});
		CHECK(g.off[(size_t)l + 1] - g.off[(size_t)l] == (int64_t)want.size(), "%s: size of list %lld", what, (long long)l);
		for (size_t j = 0; j < want.size() && g.off[(size_t)l] + (int64_t)j < g.off[(size_t)l + 1]; j++) {
			const size_t p = (size_t)g.off[(size_t)l] + j;
			CHECK(sid[p] == want[j].first && g.perm[p] == (int32_t)want[j].second, "%s: entry %zu of list %lld", what, j, (long long)l);
		}
	}
	// the subset form: positions pos of b only
	std::vector<int64_t> pos;
	for (int64_t i = 0; i < b.rows(); i += 3)
		pos.push_back(i);
	ListDirectory s = a;
	s.append_from(b, 0, &pos);
	CHECK(s.rows() == a.rows() + (int64_t)pos.size(), "%s: subset rows", what);
	for (size_t i = 0; i < pos.size(); i++)
		CHECK(s.assign[(size_t)a.rows() + i] == b.assign[(size_t)pos[i]] && s.ids[(size_t)a.rows() + i] == b.ids[(size_t)pos[i]], "%s: subset row %zu", what, i);
}

// the three subset types, written out over list_entries
static std::vector<int64_t> want_subset(const ListDirectory &d, int type, int64_t a1, int64_t a2, int64_t ntotal, bool *inverted = nullptr) {
	std::vector<int64_t> pos;
	int64_t accu_n = 0, accu_a1 = 0, accu_a2 = 0;
	for (int64_t l = 0; l < d.nlist; l++) {
		const auto e = list_entries(d, l);
		const int64_t n = (int64_t)e.size();
		if (type == 0) {
			for (auto v : e)
				if (v.first >= a1 && v.first < a2)
					pos.push_back(v.second);
		} else if (type == 1) {
			for (auto v : e)
				if (v.first % a1 == a2)
					pos.push_back(v.second);
		} else {
			const int64_t next_n = accu_n + n;
			const int64_t i1 = next_n * a1 / ntotal - accu_a1, i2 = next_n * a2 / ntotal - accu_a2;
			if (inverted && i1 > i2)
				*inverted = true;
			for (int64_t i = i1; i < i2; i++)
				pos.push_back(e[(size_t)i].second);
			accu_n = next_n, accu_a1 += i1, accu_a2 += i2;
		}
	}
	std::sort(pos.begin(), pos.end());
	return pos;
}
static void check_subset(const ListDirectory &d, const char *what) {
	const int64_t ntotal = d.rows();
	CHECK(d.subset(0, -5, 4, ntotal) == want_subset(d, 0, -5, 4, ntotal), "%s: id range", what);
	CHECK(d.subset(0, 100, 600, ntotal) == want_subset(d, 0, 100, 600, ntotal), "%s: id range 2", what);
	CHECK(d.subset(0, 7, 7, ntotal).empty(), "%s: empty id range", what);
	for (int64_t a2 : {-2, -1, 0, 1, 2})
		CHECK(d.subset(1, 3, a2, ntotal) == want_subset(d, 1, 3, a2, ntotal), "%s: id mod 3 == %lld", what, (long long)a2);
	CHECK(d.subset(3, 0, 10, ntotal).empty() && d.subset(-1, 0, 10, ntotal).empty(), "%s: other types select nothing", what);
	if (ntotal == 0) {
		CHECK(d.subset(2, 0, 0, 0).empty(), "%s: element range of nothing", what);
		return;
	}
	// the mod classes partition the listed rows (C's %: five classes once ids are negative)
	std::vector<int> hit((size_t)ntotal, 0);
	for (int64_t a2 : {-2, -1, 0, 1, 2})
		for (int64_t p : d.subset(1, 3, a2, ntotal))
			hit[(size_t)p]++;
	for (int64_t i = 0; i < ntotal; i++)
		CHECK(hit[(size_t)i] == (d.assign[(size_t)i] >= 0 ? 1 : 0), "%s: mod partition, row %lld", what, (long long)i);
	// the element ranges: the formula; and what it gives for cuts of [0, ntotal) into 1, 2, 3 and 7 parts.  The rounded cut of a list,
	// next_n a / ntotal - accu_a, is not monotone in a: a part may meet a list with i1 > i2, copies nothing of it, and its neighbours overlap
	// there (ntotal 7, three rows before a list of one, cuts 2 | 3 | 4: entries [0, 1), none, [0, 1)).  What always holds: no listed row is
	// missed, and every listed row is selected exactly once whenever no part met an inverted range
	for (int parts : {1, 2, 3, 7}) {
		std::fill(hit.begin(), hit.end(), 0);
		bool inverted = false;
		for (int k = 0; k < parts; k++) {
			const int64_t a1 = ntotal * k / parts, a2 = ntotal * (k + 1) / parts;
			const std::vector<int64_t> got = d.subset(2, a1, a2, ntotal);
			CHECK(got == want_subset(d, 2, a1, a2, ntotal, &inverted), "%s: element range [%lld, %lld)", what, (long long)a1, (long long)a2);
			CHECK(std::is_sorted(got.begin(), got.end()), "%s: element range not ascending", what);
			for (int64_t p : got)
				hit[(size_t)p]++;
		}
		CHECK(parts > 1 || !inverted, "%s: the whole range met an inverted list range", what);
		for (int64_t i = 0; i < ntotal; i++) {
			const bool listed = d.assign[(size_t)i] >= 0;
			CHECK(listed ? hit[(size_t)i] >= 1 : hit[(size_t)i] == 0, "%s: %d parts, row %lld selected %d times", what, parts, (long long)i, hit[(size_t)i]);
			CHECK(inverted || hit[(size_t)i] == (listed ? 1 : 0), "%s: %d parts without an inverted range, row %lld selected %d times", what, parts, (long long)i,
			      hit[(size_t)i]);
		}
	}
}

int main() {
	char what[128];
	for (int64_t nlist : {1, 3, 7})
		for (int64_t na : {0, 1, 40})
			for (int64_t nb : {0, 1, 40})
				for (Labels lk : {MIXED, ONE_LIST, SPARSE})
					for (int neg = 0; neg < 2; neg++) {
						const ListDirectory a = make_dir(nlist, na, lk, neg != 0), b = make_dir(nlist, nb, lk == ONE_LIST ? MIXED : lk, neg != 0);
						std::snprintf(what, sizeof what, "nlist %lld %lld+%lld labels %d neg %d", (long long)nlist, (long long)na, (long long)nb, (int)lk, neg);
						check_append(a, b, 0, what);
						check_append(a, b, 1000, what);
						check_append(a, b, -7, what);
						if (na == 0)
							check_subset(b, what);
					}
	{ // a worked example: lists [10, 11 | 12 | ] + [ | 5, 6 | 7] with add_id 100
		const int64_t la[3] = {0, 1, 0}, ia[3] = {10, 12, 11}, lb[4] = {1, 2, -1, 1}, ib[4] = {5, 7, 8, 6};
		ListDirectory a(3), b(3);
		a.append(3, la, ia, 0), b.append(4, lb, ib, 0);
		a.append_from(b, 100);
		const ListDirectory::Groups g = a.group();
		CHECK(g.off == std::vector<int64_t>({0, 2, 5, 6}), "worked example: bounds");
		CHECK(a.sorted_ids(g) == std::vector<int64_t>({10, 11, 12, 105, 106, 107}), "worked example: ids");
		CHECK(a.assign[5] == -1 && a.ids[5] == 108, "worked example: the row in no list travels as it is");
		CHECK(b.rows() == 4, "worked example: the source is unchanged");
	}
	std::printf("%s\n", fails ? "FAILED" : "ok");
	return fails ? 1 : 0;
}
"""


def test_directory_merge_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler (g++ / clang++, or CXX): a build prerequisite of this project"
    src = tmp_path / "directory_merge_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "directory_merge_main"
    # (the sanitizer runtimes linked statically where the compiler is GCC -- clang's default: the program runs as it is, whatever the
    # environment preloads)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I" + CSRC, str(src), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:]
