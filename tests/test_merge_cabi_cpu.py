"""merge_from, check_compatible_for_merge and copy_subset_to without a GPU: the three entry points are declared, documented and exported,
the Python host binds them, the faiss:: adaptor headers declare the members and the adaptor forwards them."""
import ctypes
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "duckdb-faiss-ext_amd")
COMPAT = os.path.join(PKG, "compat")

SYMBOLS = ("mvs_index_merge_from", "mvs_index_check_compatible_for_merge", "mvs_index_ivf_copy_subset_to")


def _text(*path):
    with open(os.path.join(*path)) as f:
        return " ".join(f.read().split())


def test_header_declares_the_entry_points():
    h = _text(ROOT, "include", "mi355_faiss.h")
    assert "int mvs_index_merge_from(mvs_index *ix, mvs_index *other, int64_t add_id);" in h
    assert "int mvs_index_check_compatible_for_merge(const mvs_index *ix, const mvs_index *other);" in h
    assert "int mvs_index_ivf_copy_subset_to(const mvs_index *ix, mvs_index *other, int subset_type, int64_t a1, int64_t a2);" in h


def test_header_carries_the_contract():
    with open(os.path.join(ROOT, "include", "mi355_faiss.h")) as f:  # (a comment line's leading " * " goes; a product's " * " stays)
        h = " ".join(" ".join(line.strip()[2:] if line.strip().startswith("* ") else line for line in f).split())
    for phrase in (
        "merge_from and copy_subset_to",
        "merge_from() not implemented",
        "check_compatible_for_merge() not implemented",
        "cannot set ids in FlatCodes index",
        "in other's arrival order",
        "behind ix's entries and in other's list order, with stored id + add_id",
        "nothing is re-encoded or re-assigned",
        "DEPARTURE FROM FAISS",
        "shifts other's stored ids by ix's sub-index ntotal",
        "ends with ntotal == 0",
        "DELIBERATELY STRICTER THAN FAISS",
        "equal bit for bit",
        "IDMap against IDMap2 differs",
        "other == ix is refused",
        "The 2^31-row guard of add applies to the sum",
        "is made before any state changes",
        "ivf_ids_ascending",
        "id % a1 == a2",
        "a1 <= 0 is refused",
        "i1 = next_n * a1 / ntotal - accu_a1",
        "UNVERIFIED",
        "select every listed row exactly once",
        "subset type not implemented",
        "merging across devices",
    ):
        assert phrase in h, phrase


def test_library_exports_the_entry_points():
    # (the symbol table of the built library, read without loading it: no HIP runtime is needed)
    lib = os.path.join(PKG, "libmi355faiss.so")
    assert os.path.exists(lib), "build the library first"
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", lib], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.split()}
    for s in SYMBOLS:
        assert s in names, s


def test_python_host_binds_the_entry_points():
    sys.path.insert(0, os.path.join(PKG, "pyhost"))
    import mi355_faiss as mf

    for s in SYMBOLS:
        assert s in mf.DECLARED_SYMBOLS, s
        assert isinstance(getattr(mf.lib(), s), ctypes._CFuncPtr)
    for m in ("merge_from", "check_compatible_for_merge", "copy_subset_to"):
        assert callable(getattr(mf.Index, m, None)), m
    assert (mf.Index.SUBSET_TYPE_ID_RANGE, mf.Index.SUBSET_TYPE_ID_MOD, mf.Index.SUBSET_TYPE_ELEMENT_RANGE) == (0, 1, 2)


def test_compat_headers_declare_the_members():
    ix = _text(COMPAT, "faiss", "Index.h")
    assert "virtual void merge_from(Index &otherIndex, idx_t add_id = 0);" in ix
    assert "virtual void check_compatible_for_merge(const Index &otherIndex) const;" in ix
    ivf = _text(COMPAT, "faiss", "IndexIVF.h")
    assert '#include "invlists/InvertedLists.h"' in ivf
    assert "virtual void copy_subset_to(IndexIVF &other, InvertedLists::subset_type_t subset_type, idx_t a1, idx_t a2) const;" in ivf
    inv = _text(COMPAT, "faiss", "invlists", "InvertedLists.h")
    for name, value in (("SUBSET_TYPE_ID_RANGE", 0), ("SUBSET_TYPE_ID_MOD", 1), ("SUBSET_TYPE_ELEMENT_RANGE", 2)):
        assert f"{name} = {value}," in inv
    ad = _text(COMPAT, "faiss_adaptor.cpp")
    for s in SYMBOLS:
        assert s + "(handle, " in ad, s


def test_makefile_builds_the_new_file():
    assert " merge.hip " in _text(PKG, "csrc", "Makefile")
