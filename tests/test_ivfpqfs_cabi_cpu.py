"""CPU-side checks of IndexIVFPQFastScan's boundary: the header declares the entry point and the kind and names the contract's phrases, the
built library exports the function, and the Python host lists it."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")


def test_header_declares_the_entry_point_and_the_contract():
    full = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"int\s+mvs_index_ivfpqfs_new\s*\(\s*mvs_index\s*\*\*out,\s*int d,\s*int64_t nlist,\s*int M,\s*int nbits,\s*int metric\)", src)
    assert re.search(r"#define\s+MVS_KIND_IVFPQFS\s+14\b", src)
    for phrase in ("inverted lists of 4-bit product-quantised residuals", "faiss::IndexIVFPQFastScan", "index_factory keeps refusing", "nbits == 4",
                   "M even, 2 <= M <= 128", "low nibble of byte m / 2", "floorf(fmaf(T[m][j] - lo_m, a, 0.5f))", "(((base + lo_0) + lo_1) + ...)",
                   "dis = b + (float)s / a", "then probe rank, then position in the list", "non-finite table entry or base", "do not depend on the batch",
                   "ivfpqfs_pair_block", "unknown option"):
        assert phrase in full, phrase


def test_library_exports_and_python_host_lists_it():
    import mi355_faiss as mf

    assert hasattr(ctypes.CDLL(mf.LIB_PATH), "mvs_index_ivfpqfs_new") and "mvs_index_ivfpqfs_new" in mf.DECLARED_SYMBOLS
    assert mf.KIND_IVFPQFS == 14 and callable(mf.IndexIVFPQFastScan)
