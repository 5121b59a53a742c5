"""remove_ids without a GPU: the surface is declared, documented and exported; the Python model (tests/remove_reference.py) does what
the contract says on the small cases one can check by hand; and the host plan (csrc/remove_plan.h) -- a stand-alone C++ program built
here with AddressSanitizer and UBSan and run as a process of its own, nothing is loaded into Python -- equals the model on seeded inputs
with empty lists, one-element lists, a list removed entirely and nlist = 1."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "duckdb-faiss-ext_amd")
CSRC = os.path.join(PKG, "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import remove_reference as rr  # noqa: E402


def _header():
    with open(os.path.join(ROOT, "include", "mi355_faiss.h")) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_header_declares_remove_ids():
    h = " ".join(_header().split())
    assert "int mvs_index_remove_ids(mvs_index *ix, int32_t sel_kind, const void *sel_data, int64_t sel_n, int64_t *n_removed);" in h


def test_header_carries_the_contract():
    h = " ".join(_header().replace(" * ", " ").split())
    for phrase in (
        "remove_ids not implemented for this type of index",
        "FROM MEMORY",
        "while (j < l) { if member(ids[j]) { --l; ids[j] = ids[l]; codes[j] = codes[l]; } else ++j; }",
        "[0,1,2,3,4] and members {0,1} ends as [4,3,2]",
        "DEPARTURE FROM FAISS",
        "s - #{removed r < s}",
        "not exactly 0 .. ntotal-1",
    ):
        assert phrase in h, phrase


def test_library_exports_remove_ids():
    # (the symbol table of the built library, read without loading it: no HIP runtime is needed)
    lib = os.path.join(PKG, "libmi355faiss.so")
    assert os.path.exists(lib), "build the library first"
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", lib], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    assert any(line.split()[-1] == "mvs_index_remove_ids" for line in out.splitlines() if line.split())


def test_python_host_binds_remove_ids():
    sys.path.insert(0, os.path.join(PKG, "pyhost"))
    import mi355_faiss as mf

    assert "mvs_index_remove_ids" in mf.DECLARED_SYMBOLS
    assert callable(getattr(mf.Index, "remove_ids", None))
    assert isinstance(mf.lib().mvs_index_remove_ids, ctypes._CFuncPtr)


# ---------------------------------------------------------------------------------------------------------------- the model
def _ivf_image(list_ids, d=2):
    lists = [(np.asarray(i, dtype=np.int64), np.asarray([[float(v), -float(v)] for v in i], dtype=np.float32).reshape(-1, d)) for i in list_ids]
    n = sum(len(i) for i in list_ids)
    q = {"kind": "flat", "d": d, "ntotal": len(list_ids), "metric": 1, "is_trained": True, "x": np.zeros((len(list_ids), d), np.float32)}
    return {"kind": "ivfflat", "d": d, "ntotal": n, "metric": 1, "is_trained": True, "nlist": len(list_ids), "nprobe": 1, "quantizer": q, "lists": lists}


def test_swap_loop_worked_example():
    assert rr.swap_loop([0, 1, 2, 3, 4], lambda v: v in (0, 1)) == [4, 3, 2]
    out, removed = rr.remove_image(_ivf_image([[0, 1, 2, 3, 4]]), ("batch", [0, 1]))
    assert removed == 2 and out["lists"][0][0].tolist() == [4, 3, 2]
    assert out["lists"][0][1][:, 0].tolist() == [4.0, 3.0, 2.0]  # the codes travel with their ids


def test_swap_loop_last_every_none():
    ids = [10, 11, 12, 13]
    assert rr.swap_loop(ids, lambda v: v == 13) == [0, 1, 2]
    assert rr.swap_loop(ids, lambda v: True) == []
    assert rr.swap_loop(ids, lambda v: False) == [0, 1, 2, 3]
    assert rr.swap_loop([], lambda v: True) == []
    assert rr.swap_loop([7], lambda v: v == 7) == []
    # the element swapped in is tested too: [a, b, c] minus {a, c} -> c comes to the front, goes as well, then b
    assert rr.swap_loop([1, 2, 3], lambda v: v in (1, 3)) == [1]


def test_membership_rules():
    bits = np.zeros(2, np.uint8)
    bits[0] = 0b101  # ids 0 and 2
    bits[1] = 0b10000000  # id 15
    assert rr.members(("bitmap", bits), [0, 1, 2, 15, 16, 4000, -1, -9]).tolist() == [True, False, True, True, False, False, False, False]
    assert rr.members(("batch", [5, 5, 99, -3]), [5, 6, -3]).tolist() == [True, False, True]


def test_flat_and_idmap_compact_stably():
    x = np.arange(12, dtype=np.float32).reshape(6, 2)
    flat = {"kind": "flat", "d": 2, "ntotal": 6, "metric": 1, "is_trained": True, "x": x}
    out, removed = rr.remove_image(flat, ("batch", [1, 4, 4, 77]))
    assert removed == 2 and out["ntotal"] == 4 and out["x"][:, 0].tolist() == [0.0, 4.0, 6.0, 10.0]
    out, removed = rr.remove_image(flat, ("batch", [1]), label_offset=100)  # the id is label_offset + row
    assert removed == 0 and out["ntotal"] == 6
    # a duplicate external id under IDMap: every row carrying it goes
    im = {"kind": "idmap", "d": 2, "ntotal": 6, "metric": 1, "is_trained": True, "sub": flat, "ids": np.array([9, 7, 9, 8, 7, 6])}
    out, removed = rr.remove_image(im, ("batch", [9]))
    assert removed == 2 and out["ids"].tolist() == [7, 8, 7, 6] and out["sub"]["x"][:, 0].tolist() == [2.0, 6.0, 8.0, 10.0]
    assert out["ntotal"] == 4 and out["sub"]["ntotal"] == 4


def test_idmap_over_ivf_renumbers():
    ivf = _ivf_image([[0, 3, 5], [], [1, 2, 4, 6], [7]])
    ext = np.array([100, 101, 102, 103, 104, 105, 106, 101])  # 101 twice: stored ids 1 and 7
    im = {"kind": "idmap", "d": 2, "ntotal": 8, "metric": 1, "is_trained": True, "sub": ivf, "ids": ext}
    out, removed = rr.remove_image(im, ("batch", [101, 103]))
    assert removed == 3 and out["ntotal"] == 5 and out["sub"]["ntotal"] == 5
    assert out["ids"].tolist() == [100, 102, 104, 105, 106]
    # list 0 loses stored id 3: [0, 3, 5] -> [0, 5]; list 2 loses 1: [1, 2, 4, 6] -> [6, 2, 4]; list 3 is emptied
    assert [l[0].tolist() for l in out["sub"]["lists"]] == [[0, 3], [], [4, 1, 2], []]
    # id_map[stored id] still names every survivor's external id: the code's first component is the OLD stored id
    for ids, codes in out["sub"]["lists"]:
        for s, c in zip(ids.tolist(), codes[:, 0].tolist()):
            assert out["ids"][s] == ext[int(c)]
    rows, stored, external = rr.survivors(out)
    assert stored.tolist() == [0, 3, 4, 1, 2] and external.tolist() == [100, 105, 106, 102, 104] and rows[:, 0].tolist() == [0.0, 5.0, 6.0, 2.0, 4.0]


def test_idmap_over_ivf_refuses_foreign_ids():
    ivf = _ivf_image([[0, 2], [5]])
    im = {"kind": "idmap", "d": 2, "ntotal": 3, "metric": 1, "is_trained": True, "sub": ivf, "ids": np.array([1, 2, 3])}
    try:
        rr.remove_image(im, ("batch", [1]))
    except ValueError as e:
        assert "not exactly 0 .. ntotal-1" in str(e)
    else:
        raise AssertionError("accepted")


# ---------------------------------------------------------------------------------------------------------------- the host plan
PROGRAM = r"""
#include "remove_plan.h"
#include <cstdio>
#include <cstdlib>
using namespace mvs;
// stdin: nlist n renumber sel_kind sel_n | assign[n] | ids[n] | selector (bitmap bytes or batch ids) | idmap[n] when renumber
// stdout: removed nkeep | perm | assign | ids
int main() {
	long long nlist, n, renumber, kind, seln;
	if (std::scanf("%lld %lld %lld %lld %lld", &nlist, &n, &renumber, &kind, &seln) != 5)
		return 2;
	std::vector<int32_t> assign((size_t)n);
	std::vector<int64_t> ids((size_t)n), idmap;
	for (auto &v : assign) { long long t; if (std::scanf("%lld", &t) != 1) return 2; v = (int32_t)t; }
	for (auto &v : ids) { long long t; if (std::scanf("%lld", &t) != 1) return 2; v = t; }
	std::vector<uint8_t> bits;
	std::vector<int64_t> batch;
	for (long long i = 0; i < seln; ++i) {
		long long t;
		if (std::scanf("%lld", &t) != 1) return 2;
		if (kind == 1) bits.push_back((uint8_t)t); else batch.push_back(t);
	}
	const RemoveSelector rs((int)kind, kind == 1 ? (const void *)bits.data() : (const void *)batch.data(), seln);
	std::vector<uint8_t> keep((size_t)n);
	std::vector<int64_t> renum;
	if (renumber) {
		idmap.resize((size_t)n);
		for (auto &v : idmap) { long long t; if (std::scanf("%lld", &t) != 1) return 2; v = t; }
		if (!remove_ids_are_permutation(ids)) { std::printf("refused\n"); return 0; }
		std::vector<uint8_t> kb((size_t)n);
		for (long long s = 0; s < n; ++s) kb[(size_t)s] = rs.member(idmap[(size_t)s]) ? 0 : 1;
		for (long long i = 0; i < n; ++i) keep[(size_t)i] = kb[(size_t)ids[(size_t)i]];
		renum = remove_renumber(kb);
	} else
		for (long long i = 0; i < n; ++i) keep[(size_t)i] = rs.member(ids[(size_t)i]) ? 0 : 1;
	IvfRemovePlan p;
	ivf_remove_plan(nlist, assign, ids, keep, renumber ? &renum : nullptr, p);
	std::printf("%lld %zu\n", (long long)p.removed, p.perm.size());
	for (auto v : p.perm) std::printf("%d ", v);
	std::printf("\n");
	for (auto v : p.assign) std::printf("%d ", v);
	std::printf("\n");
	for (auto v : p.ids) std::printf("%lld ", (long long)v);
	std::printf("\n");
	return 0;
}
"""


def _build_plan_program(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler (g++ / clang++, or CXX): a build prerequisite of this project"
    src = tmp_path / "remove_plan_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "remove_plan_main"
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                       ["-I" + CSRC, str(src), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return str(exe)


def _run_plan(exe, nlist, assign, ids, sel, idmap=None):
    kind = 1 if sel[0] == "bitmap" else 2
    data = np.asarray(sel[1]).astype(np.int64).tolist()
    words = [nlist, len(assign), 1 if idmap is not None else 0, kind, len(data)] + list(assign) + list(ids) + data + (list(idmap) if idmap is not None else [])
    r = subprocess.run([exe], input=" ".join(str(int(w)) for w in words), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    lines = r.stdout.split("\n")
    if lines[0].strip() == "refused":
        return None
    removed, nkeep = (int(v) for v in lines[0].split())
    perm, asg, nid = ([int(v) for v in lines[i].split()] for i in (1, 2, 3))
    assert len(perm) == len(asg) == len(nid) == nkeep
    return removed, perm, asg, nid


def _model_plan(nlist, assign, ids, sel, idmap=None):
    """the model on the same input: lists in arrival order -> swap loops -> list-major arrival order"""
    assign, ids = np.asarray(assign), np.asarray(ids, dtype=np.int64)
    pos = [np.nonzero(assign == l)[0] for l in range(nlist)]
    orders, new_ids, removed, _ = rr.remove_lists([ids[p] for p in pos], sel, idmap)
    perm = [int(pos[l][j]) for l in range(nlist) for j in orders[l]]
    asg = [l for l in range(nlist) for _ in orders[l]]
    nid = [int(v) for l in range(nlist) for v in new_ids[l]]
    return removed, perm, asg, nid


def test_plan_program_under_sanitizers(tmp_path):
    exe = _build_plan_program(tmp_path)
    rng = np.random.default_rng(7)
    # the worked example, nlist = 1
    assert _run_plan(exe, 1, [0] * 5, [0, 1, 2, 3, 4], ("batch", [0, 1])) == (2, [4, 3, 2], [0, 0, 0], [4, 3, 2])
    cases = 0
    for nlist, n in ((1, 1), (1, 40), (5, 0), (5, 3), (8, 200), (16, 333), (3, 64)):
        for trial in range(3):
            # lists 0 and 1 (where they exist) stay empty / hold one row; the last list is removed entirely in trial 0
            assign = rng.integers(min(2, nlist - 1), nlist, size=n)
            if n > 2 and nlist > 2:
                assign[n // 2] = 1
            ids = rng.permutation(n).astype(np.int64)
            gone = ids[rng.random(n) < (0.1, 0.5, 0.9)[trial]]
            if trial == 0:
                gone = np.concatenate([gone, ids[assign == nlist - 1]])
            batch = ("batch", np.concatenate([gone, gone[:3], [10**12, -5]]).astype(np.int64))  # duplicates and absent ids
            bits = np.zeros(max(n // 16, 1), np.uint8)  # shorter than ntotal / 8: the ids beyond it are no members
            for v in gone.tolist():
                if (v >> 3) < bits.size:
                    bits[v >> 3] |= 1 << (v & 7)
            for sel in (batch, ("bitmap", bits)):
                assert _run_plan(exe, nlist, assign.tolist(), ids.tolist(), sel) == _model_plan(nlist, assign, ids, sel)
                # under IDMap: external ids with duplicates, membership through id_map, survivors renumbered
                ext = rng.integers(0, max(n // 2, 1), size=n).astype(np.int64)
                esel = ("batch", ext[rng.random(n) < 0.3]) if sel[0] == "batch" else sel
                got = _run_plan(exe, nlist, assign.tolist(), ids.tolist(), esel, ext.tolist())
                assert got == _model_plan(nlist, assign, ids, esel, ext)
                cases += 2
    # stored ids that are no permutation of 0 .. n-1 are refused under IDMap
    assert _run_plan(exe, 2, [0, 1, 1], [0, 2, 5], ("batch", [1]), [1, 2, 3]) is None
    assert _run_plan(exe, 2, [0, 1, 1], [0, 1, 1], ("batch", [1]), [1, 2, 3]) is None
    assert cases >= 80
