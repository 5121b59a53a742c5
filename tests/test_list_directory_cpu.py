"""The host directory of the inverted lists (csrc/list_directory.h: ListDirectory) and the removal plan over it (csrc/remove_plan.h): a
stand-alone C++ program, built here with AddressSanitizer and UBSan and run as a process of its own (nothing is loaded into Python).  The
program holds a literal copy of the three loops the directory replaced -- IVFFlatIndex::build_lists's and CodedListsIndex::build_lists's
groupings and ivf_remove_plan's as it was -- and checks group(), the sorted ids, adopt_image over to_lists and the plan's perm / assign /
ids / removed against them.  Shapes: nlist 1, 3 and 7; 0, 1 and 40 rows; labels that include -1 (and, for append's clamp, values outside
[0, nlist)); empty lists; every row in one list; explicit ids with duplicates; implicit ids from a non-zero first id.  A round trip
directory -> lists -> adopt_image must give the list-major order whose group() has the same bounds and sorted ids."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "duckdb-faiss-ext_amd", "csrc")

PROGRAM = r"""
#include "remove_plan.h"
#include <cstdio>
#include <cstdlib>
using namespace mvs;
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

// ---- the loops as they were ------------------------------------------------------------------------------------------------------
struct OldView {
	std::vector<int64_t> list_off, sid;
	std::vector<int32_t> perm;
	int64_t nsorted = 0;
};
// IVFFlatIndex::build_lists (csrc/ivf.hip)
static OldView old_ivf_build_lists(int64_t nlist, int64_t ntotal, const std::vector<int32_t> &assign_h, const std::vector<int64_t> &ids_h) {
	std::vector<int64_t> list_off;
	int64_t nsorted;
	list_off.assign((size_t)nlist + 1, 0);
	for (int64_t i = 0; i < ntotal; i++) {
		const int32_t l = assign_h[(size_t)i];
		if (l >= 0)
			list_off[(size_t)l + 1]++;
	}
	for (int64_t l = 0; l < nlist; l++)
		list_off[(size_t)l + 1] += list_off[(size_t)l];
	nsorted = list_off[(size_t)nlist];
	std::vector<int64_t> cursor(list_off.begin(), list_off.end() - 1);
	std::vector<int32_t> perm((size_t)nsorted);
	std::vector<int64_t> sid((size_t)nsorted);
	for (int64_t i = 0; i < ntotal; i++) {
		const int32_t l = assign_h[(size_t)i];
		if (l < 0)
			continue;
		const int64_t p = cursor[(size_t)l]++;
		perm[(size_t)p] = (int32_t)i;
		sid[(size_t)p] = ids_h[(size_t)i];
	}
	OldView v;
	v.list_off = list_off, v.sid = sid, v.perm = perm, v.nsorted = nsorted;
	return v;
}
// CodedListsIndex::build_lists, the branch with a quantiser (csrc/coded_lists.hip); top_rows / max_list are the caller's still
static OldView old_coded_build_lists(int64_t nlist, int64_t ntotal, const std::vector<int32_t> &assign_h, const std::vector<int64_t> &ids_h) {
	std::vector<int64_t> list_off, sid_h;
	int64_t nsorted;
	list_off.assign((size_t)nlist + 1, 0);
	for (int64_t i = 0; i < ntotal; i++)
		if (assign_h[(size_t)i] >= 0)
			list_off[(size_t)assign_h[(size_t)i] + 1]++;
	for (int64_t l = 0; l < nlist; l++)
		list_off[(size_t)l + 1] += list_off[(size_t)l];
	nsorted = list_off[(size_t)nlist];
	std::vector<int64_t> cursor(list_off.begin(), list_off.end() - 1);
	std::vector<int32_t> perm((size_t)nsorted);
	sid_h.assign((size_t)nsorted, 0);
	for (int64_t i = 0; i < ntotal; i++) {
		const int32_t l = assign_h[(size_t)i];
		if (l < 0)
			continue;
		const int64_t p = cursor[(size_t)l]++;
		perm[(size_t)p] = (int32_t)i;
		sid_h[(size_t)p] = ids_h[(size_t)i];
	}
	OldView v;
	v.list_off = list_off, v.sid = sid_h, v.perm = perm, v.nsorted = nsorted;
	return v;
}
// ivf_remove_plan (csrc/remove_plan.h) before it called ListDirectory::group
static void old_ivf_remove_plan(int64_t nlist, const std::vector<int32_t> &assign_h, const std::vector<int64_t> &ids_h, const std::vector<uint8_t> &keep,
                                const std::vector<int64_t> *renum, IvfRemovePlan &out) {
	const int64_t n = (int64_t)assign_h.size();
	std::vector<int64_t> off((size_t)nlist + 1, 0);
	for (int64_t i = 0; i < n; ++i)
		if (assign_h[(size_t)i] >= 0)
			off[(size_t)assign_h[(size_t)i] + 1]++;
	for (int64_t l = 0; l < nlist; ++l)
		off[(size_t)l + 1] += off[(size_t)l];
	std::vector<int32_t> pos((size_t)off[(size_t)nlist]); // arrival positions grouped by list, arrival order inside a list
	{
		std::vector<int64_t> cur(off.begin(), off.end() - 1);
		for (int64_t i = 0; i < n; ++i)
			if (assign_h[(size_t)i] >= 0)
				pos[(size_t)cur[(size_t)assign_h[(size_t)i]]++] = (int32_t)i;
	}
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

// ---- cases -----------------------------------------------------------------------------------------------------------------------
static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { // xorshift64
	rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
	return rng_state;
}
enum Labels { MIXED, ONE_LIST, SPARSE }; // -1 among the labels | every row in list nlist - 1 | only lists 0 and nlist - 1 (the others stay empty)
enum Ids { IMPLICIT, DUPLICATES, PERMUTATION };

static void one_case(int64_t nlist, int64_t n, Labels lab_kind, Ids id_kind) {
	char what[96];
	std::snprintf(what, sizeof what, "nlist %lld rows %lld labels %d ids %d", (long long)nlist, (long long)n, (int)lab_kind, (int)id_kind);
	std::vector<int64_t> labels((size_t)n), ids_in((size_t)n);
	for (int64_t i = 0; i < n; ++i) {
		if (lab_kind == ONE_LIST)
			labels[(size_t)i] = nlist - 1;
		else if (lab_kind == SPARSE)
			labels[(size_t)i] = rnd() % 2 ? 0 : nlist - 1;
		else
			labels[(size_t)i] = rnd() % 5 == 0 ? -1 : (int64_t)(rnd() % (uint64_t)nlist);
		ids_in[(size_t)i] = id_kind == DUPLICATES ? (int64_t)(rnd() % 7) * 1000 - 2000 : i;
	}
	if (id_kind == PERMUTATION) // 0 .. n-1, each once, shuffled: what an IVF kind under IDMap stores
		for (int64_t i = n - 1; i > 0; --i)
			std::swap(ids_in[(size_t)i], ids_in[(size_t)(rnd() % (uint64_t)(i + 1))]);
	const int64_t first_id = 1000003;
	// the directory, filled in two blocks by the one append
	ListDirectory dir(nlist);
	const int64_t n0 = n / 3;
	const bool implicit = id_kind == IMPLICIT;
	dir.reserve(n);
	dir.append(n0, labels.data(), implicit ? nullptr : ids_in.data(), first_id);
	dir.append(n - n0, labels.data() + n0, implicit ? nullptr : ids_in.data() + n0, first_id + n0);
	// ... and what the two classes kept before: IVFFlatIndex cast the label, the coded kinds clamped it (the same for -1 .. nlist - 1)
	std::vector<int32_t> assign_h;
	std::vector<int64_t> ids_h;
	for (int64_t i = 0; i < n; ++i) {
		assign_h.push_back((int32_t)labels[(size_t)i]);
		ids_h.push_back(implicit ? first_id + i : ids_in[(size_t)i]);
	}
	CHECK(dir.rows() == n && dir.assign == assign_h && dir.ids == ids_h, "%s: append", what);

	const OldView a = old_ivf_build_lists(nlist, n, assign_h, ids_h), b = old_coded_build_lists(nlist, n, assign_h, ids_h);
	const ListDirectory::Groups g = dir.group();
	const std::vector<int64_t> sid = dir.sorted_ids(g);
	CHECK(g.off == a.list_off && g.perm == a.perm && sid == a.sid && (int64_t)g.perm.size() == a.nsorted, "%s: group() against IVFFlatIndex::build_lists", what);
	CHECK(g.off == b.list_off && g.perm == b.perm && sid == b.sid && (int64_t)g.perm.size() == b.nsorted, "%s: group() against CodedListsIndex::build_lists", what);
	CHECK((int64_t)g.off.size() == nlist + 1 && g.off[0] == 0, "%s: off", what);
	if (lab_kind == ONE_LIST)
		CHECK(g.off[(size_t)nlist - 1] == 0 && g.off[(size_t)nlist] == n, "%s: every row in the last list", what);

	// directory -> lists -> adopt_image: list-major, the same bounds and sorted ids, the positions of a list ascending
	std::vector<std::vector<int64_t>> list_ids;
	std::vector<std::vector<int32_t>> list_pos;
	dir.to_lists(list_ids, list_pos);
	CHECK((int64_t)list_ids.size() == nlist && (int64_t)list_pos.size() == nlist, "%s: to_lists sizes", what);
	for (int64_t l = 0; l < nlist; ++l) {
		CHECK(list_ids[(size_t)l] == std::vector<int64_t>(sid.begin() + g.off[(size_t)l], sid.begin() + g.off[(size_t)l + 1]), "%s: ids of list %lld", what, (long long)l);
		CHECK(list_pos[(size_t)l] == std::vector<int32_t>(g.perm.begin() + g.off[(size_t)l], g.perm.begin() + g.off[(size_t)l + 1]), "%s: positions of list %lld", what, (long long)l);
		for (size_t j = 0; j < list_pos[(size_t)l].size(); ++j)
			CHECK(assign_h[(size_t)list_pos[(size_t)l][j]] == l && (j == 0 || list_pos[(size_t)l][j] > list_pos[(size_t)l][j - 1]), "%s: list %lld entry %zu", what, (long long)l, j);
	}
	ListDirectory img(nlist);
	const int64_t list0 = 0;
	img.append(1, &list0, nullptr, 5); // (adopt_image replaces what the directory held)
	const int64_t nimg = img.adopt_image(list_ids);
	CHECK(nimg == a.nsorted && img.rows() == nimg && (int64_t)img.assign.size() == nimg, "%s: adopt_image's row count", what);
	CHECK(img.ids == sid, "%s: adopt_image's ids are the sorted ids", what);
	for (int64_t r = 1; r < nimg; ++r)
		CHECK(img.assign[(size_t)r] >= img.assign[(size_t)r - 1], "%s: adopt_image is not list-major at row %lld", what, (long long)r);
	const ListDirectory::Groups gi = img.group();
	CHECK(gi.off == g.off && img.sorted_ids(gi) == sid, "%s: the image's group()", what);
	for (int64_t r = 0; r < nimg; ++r)
		CHECK(gi.perm[(size_t)r] == (int32_t)r, "%s: the image's perm is not the identity at %lld", what, (long long)r);

	// the removal plan, plain and renumbered (IDMap: stored ids 0 .. n-1), against the loop as it was; then adopted
	for (int pass = 0; pass < 3; ++pass) { // keep about two thirds | nothing | everything
		std::vector<uint8_t> keep((size_t)n);
		for (int64_t i = 0; i < n; ++i)
			keep[(size_t)i] = pass == 0 ? (rnd() % 3 != 0) : (pass == 2);
		for (int renumber = 0; renumber <= (id_kind == PERMUTATION ? 1 : 0); ++renumber) {
			std::vector<int64_t> renum;
			if (renumber) {
				std::vector<uint8_t> keep_by_id((size_t)n);
				for (int64_t i = 0; i < n; ++i)
					keep_by_id[(size_t)ids_h[(size_t)i]] = keep[(size_t)i];
				renum = remove_renumber(keep_by_id);
			}
			IvfRemovePlan want, got;
			old_ivf_remove_plan(nlist, assign_h, ids_h, keep, renumber ? &renum : nullptr, want);
			ivf_remove_plan(dir.nlist, dir.assign, dir.ids, keep, renumber ? &renum : nullptr, got);
			CHECK(got.perm == want.perm && got.assign == want.assign && got.ids == want.ids && got.removed == want.removed, "%s: plan, pass %d renumber %d", what,
			      pass, renumber);
			ListDirectory after = dir;
			after.adopt(std::move(got));
			CHECK(after.nlist == nlist && after.assign == want.assign && after.ids == want.ids && after.rows() == n - want.removed, "%s: adopt, pass %d", what, pass);
		}
	}
}

int main() {
	for (int64_t nlist : {1, 3, 7})
		for (int64_t n : {0, 1, 40})
			for (Labels lk : {MIXED, ONE_LIST, SPARSE})
				for (Ids ik : {IMPLICIT, DUPLICATES, PERMUTATION})
					one_case(nlist, n, lk, ik);
	{ // append's clamp: a label outside [0, nlist) is "no list", whatever its value
		const int64_t labels[6] = {2, -1, 3, -7, 0, (int64_t)1 << 32};
		ListDirectory d(3);
		d.append(6, labels, nullptr, -2);
		CHECK(d.assign == std::vector<int32_t>({2, -1, -1, -1, 0, -1}), "clamp");
		CHECK(d.ids == std::vector<int64_t>({-2, -1, 0, 1, 2, 3}), "implicit ids from a negative first id");
		const ListDirectory::Groups g = d.group();
		CHECK(g.off == std::vector<int64_t>({0, 1, 1, 2}) && g.perm == std::vector<int32_t>({4, 0}), "group() after the clamp");
	}
	std::printf("%s\n", fails ? "FAILED" : "ok");
	return fails ? 1 : 0;
}
"""


def test_list_directory_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler (g++ / clang++, or CXX): a build prerequisite of this project"
    src = tmp_path / "list_directory_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "list_directory_main"
    # (the sanitizer runtimes linked statically where the compiler is GCC -- clang's default: the program runs as it is, whatever the
    # environment preloads)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I" + CSRC, str(src), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:]
