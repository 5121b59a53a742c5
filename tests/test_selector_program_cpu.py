"""Selector programs on the host (include/mi355_faiss.h "selector programs"; csrc/selector_program.h): the header states the contract, and
a stand-alone C++ program -- built here with AddressSanitizer and UBSan and run as a process of its own, nothing is loaded into Python --
feeds sel_program_validate the malformed programs the contract lists and compares sel_program_member with the numpy model of
tests/selector_reference.py on random trees of depth <= 6 over ids that include negatives, 0, 2^40, INT64_MIN / INT64_MAX and the ids one
past a bitmap's end."""

import os
import shutil
import subprocess

import numpy as np

import selector_reference as selr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "duckdb-faiss-ext_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")


def test_header_states_the_contract():
    text = open(HEADER).read()
    flat = " ".join(text.split())
    assert "#define MVS_SEL_PROGRAM 3" in text
    assert "typedef struct mvs_sel_node {" in text and "} mvs_sel_node;" in text
    for field in ("int32_t op;", "int32_t reserved;", "const void *data;", "int64_t n;", "int64_t imin, imax;"):
        assert field in text[text.index("typedef struct mvs_sel_node {"):text.index("} mvs_sel_node;")], field
    for op in ("ALL", "BITMAP", "BATCH", "ARRAY", "RANGE", "NOT", "AND", "OR", "XOR"):
        assert "#define MVS_SELOP_" + op + " " in text, op
    assert "postfix" in flat and "bit for bit" in flat and "FROM MEMORY" in flat
    assert "sel_bitmap_cap_bytes" in flat and "sel_lowered" in flat and "sel_admitted" in flat


PROGRAM = r"""
#include "selector_program.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace mvs;
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static mvs_sel_node node(int op, const void *data = nullptr, int64_t n = 0, int64_t imin = 0, int64_t imax = 0) {
	mvs_sel_node nd;
	memset(&nd, 0, sizeof nd);
	nd.op = op, nd.data = data, nd.n = n, nd.imin = imin, nd.imax = imax;
	return nd;
}
static void expect_error(const char *what, const std::vector<mvs_sel_node> &p, int64_t n, const char *node_text, const char *reason) {
	const std::string e = sel_program_validate(p.empty() ? nullptr : p.data(), n);
	CHECK(!e.empty() && e.find(node_text) != std::string::npos && e.find(reason) != std::string::npos, "%s: got \"%s\", want \"%s\" and \"%s\"", what,
	      e.c_str(), node_text, reason);
}

static void malformed() {
	const int64_t ids[2] = {1, 2};
	const mvs_sel_node all = node(MVS_SELOP_ALL), rng = node(MVS_SELOP_RANGE, nullptr, 0, 0, 5);
	expect_error("zero nodes", {}, 0, "node 0", "empty");
	expect_error("unknown op 0", {all, node(0), node(MVS_SELOP_AND)}, 3, "node 1", "unknown op 0");
	expect_error("unknown op 10", {node(10)}, 1, "node 0", "unknown op 10");
	expect_error("NOT on nothing", {node(MVS_SELOP_NOT)}, 1, "node 0", "stack underflow");
	expect_error("AND on one", {all, node(MVS_SELOP_AND)}, 2, "node 1", "stack underflow");
	expect_error("XOR after the stack ran out", {all, rng, node(MVS_SELOP_OR), node(MVS_SELOP_XOR)}, 4, "node 3", "stack underflow");
	expect_error("two values left", {all, rng}, 2, "node 1", "2 values left");
	expect_error("three values left", {all, rng, all, node(MVS_SELOP_NOT)}, 4, "node 3", "3 values left");
	expect_error("n < 0", {all, node(MVS_SELOP_BATCH, ids, -1), node(MVS_SELOP_AND)}, 3, "node 1", "n < 0");
	expect_error("bitmap n < 0", {node(MVS_SELOP_BITMAP, ids, -5)}, 1, "node 0", "n < 0");
	expect_error("NULL data", {node(MVS_SELOP_ARRAY, nullptr, 2)}, 1, "node 0", "NULL data with n > 0");
	std::vector<mvs_sel_node> big;
	for (int i = 0; i < 33; ++i)
		big.push_back(all);
	for (int i = 0; i < 32; ++i)
		big.push_back(node(MVS_SELOP_OR));
	expect_error("65 nodes", big, 65, "node 64", "more than 64 nodes");
	// well formed: 64 nodes (the stack 32 deep, then emptied); NULL data with n == 0
	std::vector<mvs_sel_node> deep;
	for (int i = 0; i < 32; ++i)
		deep.push_back(i == 7 ? rng : all);
	for (int i = 0; i < 31; ++i)
		deep.push_back(node(MVS_SELOP_AND));
	deep.push_back(node(MVS_SELOP_NOT));
	CHECK(deep.size() == 64 && sel_program_validate(deep.data(), 64).empty(), "64 nodes are accepted: %s", sel_program_validate(deep.data(), 64).c_str());
	SelProgram pk;
	sel_program_pack(deep.data(), 64, pk);
	CHECK(!sel_program_member(pk, 3) && sel_program_member(pk, 5) && sel_program_member(pk, -1), "NOT(AND(31 x ALL, RANGE [0, 5)))");
	const std::vector<mvs_sel_node> empty_batch = {node(MVS_SELOP_BATCH, nullptr, 0)};
	CHECK(sel_program_validate(empty_batch.data(), 1).empty(), "an empty batch is well formed");
	sel_program_pack(empty_batch.data(), 1, pk);
	CHECK(!sel_program_member(pk, 0) && pk.blob.empty(), "an empty batch admits nothing");
	const std::vector<mvs_sel_node> empty_bitmap_not = {node(MVS_SELOP_BITMAP, nullptr, 0), node(MVS_SELOP_NOT)};
	sel_program_pack(empty_bitmap_not.data(), 2, pk);
	CHECK(sel_program_member(pk, 0) && sel_program_member(pk, INT64_MIN), "NOT(empty bitmap) admits everything");
}

// the cases file: ncases; per case: nnodes, then per node "op n imin imax" and n values (a bitmap's bytes, a list's ids); then nids, the ids
// and the expected membership as nids digits
static int from_file(const char *path) {
	FILE *f = fopen(path, "r");
	if (!f)
		return -1;
	long long ncases = 0;
	if (fscanf(f, "%lld", &ncases) != 1)
		return -1;
	for (long long c = 0; c < ncases; ++c) {
		long long nn = 0;
		if (fscanf(f, "%lld", &nn) != 1)
			return -1;
		std::vector<mvs_sel_node> nodes((size_t)nn);
		std::vector<std::vector<uint8_t>> bytes((size_t)nn);
		std::vector<std::vector<int64_t>> lists((size_t)nn);
		for (long long i = 0; i < nn; ++i) {
			long long op, n, imin, imax;
			if (fscanf(f, "%lld %lld %lld %lld", &op, &n, &imin, &imax) != 4)
				return -1;
			for (long long j = 0; j < n; ++j) {
				long long v;
				if (fscanf(f, "%lld", &v) != 1)
					return -1;
				if (op == MVS_SELOP_BITMAP)
					bytes[(size_t)i].push_back((uint8_t)v);
				else
					lists[(size_t)i].push_back((int64_t)v);
			}
			// (exactly n elements behind the pointer: the sanitizer sees a read past either end)
			const void *data = op == MVS_SELOP_BITMAP ? (const void *)bytes[(size_t)i].data() : (const void *)lists[(size_t)i].data();
			nodes[(size_t)i] = node((int)op, n > 0 ? data : nullptr, n, imin, imax);
		}
		const std::string e = sel_program_validate(nodes.data(), nn);
		CHECK(e.empty(), "case %lld: %s", c, e.c_str());
		if (!e.empty())
			return -1;
		SelProgram pk;
		sel_program_pack(nodes.data(), nn, pk);
		long long nids = 0;
		if (fscanf(f, "%lld", &nids) != 1)
			return -1;
		std::vector<int64_t> ids((size_t)nids);
		for (long long i = 0; i < nids; ++i) {
			long long v;
			if (fscanf(f, "%lld", &v) != 1)
				return -1;
			ids[(size_t)i] = v;
		}
		std::vector<char> want((size_t)nids + 1);
		if (fscanf(f, "%s", want.data()) != 1 && nids > 0)
			return -1;
		int bad = 0;
		for (long long i = 0; i < nids; ++i)
			if (sel_program_member(pk, ids[(size_t)i]) != (want[(size_t)i] == '1') && ++bad <= 3)
				CHECK(false, "case %lld: id %lld: member says %d, the model %c", c, (long long)ids[(size_t)i], (int)sel_program_member(pk, ids[(size_t)i]),
				      want[(size_t)i]);
	}
	fclose(f);
	return (int)ncases;
}

int main(int argc, char **argv) {
	malformed();
	const int ncases = argc > 1 ? from_file(argv[1]) : -1;
	CHECK(ncases > 0, "the cases file could not be read");
	std::printf("%d cases\n%s\n", ncases, fails ? "FAILED" : "ok");
	return fails ? 1 : 0;
}
"""


def _cases(rng):
    i64 = np.iinfo(np.int64)
    cases = []
    for c in range(60):
        base = rng.integers(0, 5000, 200)
        pool = np.concatenate([base, -rng.integers(1, 5000, 40), [0, 1 << 40, (1 << 40) + 1, i64.min, i64.max, i64.min + 1, i64.max - 1, -1]]).astype(np.int64)
        tree = selr.random_tree(rng, pool, 1 + c % 6)
        nodes = selr.postfix(tree)
        assert len(nodes) <= 64
        ids = [pool, rng.integers(-6000, 6000, 100)]
        for op, a, _, _ in nodes:  # the ids around a bitmap's end, and around every bound and list entry
            if op == selr.OPS["bitmap"]:
                ids.append(np.arange(8 * a.size - 9, 8 * a.size + 9))
            elif a is not None and a.size:
                ids.append(a[:5].astype(object) + 1)
        for nd in nodes:
            if nd[0] == selr.OPS["range"]:
                ids.append(np.array([nd[2] - 1, nd[2], nd[3] - 1, nd[3]], dtype=object))
        flat = np.array([int(v) for part in ids for v in np.asarray(part).ravel() if i64.min <= int(v) <= i64.max], dtype=np.int64)
        cases.append((tree, nodes, flat))
    return cases


def test_validate_and_member_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler (g++ / clang++, or CXX): a build prerequisite of this project"
    cases = _cases(np.random.default_rng(2024))
    assert max(len(n) for _, n, _ in cases) >= 10 and any(m.any() and not m.all() for m in (selr.mask(i, t) for t, _, i in cases))
    lines = [str(len(cases))]
    for tree, nodes, ids in cases:
        lines.append(str(len(nodes)))
        for op, a, imin, imax in nodes:
            vals = [] if a is None else [int(v) for v in a]
            lines.append(" ".join(str(v) for v in [op, len(vals), imin, imax] + vals))
        lines.append(str(ids.size))
        lines.append(" ".join(str(int(v)) for v in ids))
        lines.append("".join("1" if m else "0" for m in selr.mask(ids, tree)))
    data = tmp_path / "selector_cases.txt"
    data.write_text("\n".join(lines) + "\n")
    src = tmp_path / "selector_program_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "selector_program_main"
    # (the sanitizer runtimes linked statically where the compiler is GCC -- clang's default: the program runs as it is, whatever the
    # environment preloads)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I" + CSRC, str(src), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(exe), str(data)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "%d cases" % len(cases) in r.stdout, r.stdout[-4000:]
