"""CPU-side checks of the range-search boundary: the header declares the six functions and the contract's key phrases, the built
library exports them, the Python host lists them, and the CPU model (tests/range_reference.py) agrees with the oracle's own search."""
import ctypes
import os
import re

import numpy as np
import pytest

import range_reference as rr
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")
RANGE_FUNCTIONS = {
    "mvs_index_range_search": "int",
    "mvs_range_result_nq": "int64_t",
    "mvs_range_result_lims": r"const\s+int64_t\s*\*",
    "mvs_range_result_distances": r"const\s+float\s*\*",
    "mvs_range_result_labels": r"const\s+int64_t\s*\*",
    "mvs_range_result_free": "void",
}
L2, IP = rr.L2, rr.IP


def test_header_declares_the_range_functions_and_contract():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+mvs_range_result\s+mvs_range_result\s*;", src)
    for name, ret in RANGE_FUNCTIONS.items():
        assert re.search(r"%s\s*%s\s*\(" % (ret, name), src), name
    full = open(HEADER).read()
    for phrase in ("range search", "strict", "range search not implemented", "probe rank", "range_stream_cap", "range_mfma", "range_rescans",
                   "RangeSearchBlockResultHandler", "FROM MEMORY"):
        assert phrase in full, phrase


def test_library_exports_the_range_functions():
    import mi355_faiss as mf

    L = ctypes.CDLL(mf.LIB_PATH)
    missing = [n for n in RANGE_FUNCTIONS if not hasattr(L, n)]
    assert not missing, missing


def test_python_host_lists_the_range_functions():
    import mi355_faiss as mf

    for name in RANGE_FUNCTIONS:
        assert name in mf.DECLARED_SYMBOLS, name
    assert callable(mf.Index.range_search)


def _data(seed, n, d, nq):
    rng = np.random.default_rng(seed)
    xb = rng.random((n, d), dtype=np.float32)
    xb[n // 2 :: 7] = xb[: len(xb[n // 2 :: 7])]  # duplicated rows: equal distances
    xq = rng.random((nq, d), dtype=np.float32)
    xq[:3] = xb[[1, n // 3, n - 1]]
    return xb, xq


@pytest.mark.parametrize("metric,nq", [(L2, 7), (L2, 33), (IP, 7), (IP, 33)])
def test_model_agrees_with_the_oracle_search(metric, nq):
    """for each query, the first entries of orc.flat_search(k) whose distance is inside the radius are the model's k best hits -- on the
    per-pair branch (nq < 20) and on the BLAS branch (nq >= 20)"""
    n, d, k = 300, 24, 40
    xb, xq = _data(11 + nq, n, d, nq)
    dis = rr.flat_matrix(metric, xb, xq)
    radius = np.float32(np.quantile(dis, 0.08 if metric == L2 else 0.92))
    lims, D, I = rr.flat_range(metric, xb, xq, radius)
    Do, Io = orc.flat_search(metric, xb, xq, k)
    some = 0
    for q in range(nq):
        inside = rr.hits(metric, Do[q], radius) & (Io[q] >= 0)
        want_D, want_I = Do[q][inside], Io[q][inside]
        got_D, got_I = D[lims[q] : lims[q + 1]], I[lims[q] : lims[q + 1]]
        assert np.array_equal(np.sort(got_I), got_I), "hits of a query are in ascending row order"
        # the model's k best in the search's value order; equal values may be ordered differently, so compare values and label sets
        order = np.lexsort((got_I, got_D if metric == L2 else -got_D))[:k]
        assert np.array_equal(got_D[order][: want_D.size].view(np.uint32), want_D.view(np.uint32)), q
        if want_D.size < k:  # the search saw every hit
            assert got_D.size == want_D.size and set(got_I.tolist()) == set(want_I.tolist()), q
        some += want_D.size
    assert some > nq  # (the radius admits something)


def test_the_two_l2_branches_differ_and_the_ip_branches_agree():
    xb, xq = _data(5, 200, 64, 8)
    a, b = rr.all_distances(L2, xb, xq, orc.PATH_PAIR), rr.all_distances(L2, xb, xq, orc.PATH_BLAS)
    assert (a.view(np.uint32) != b.view(np.uint32)).mean() > 0.25
    a, b = rr.all_distances(IP, xb, xq, orc.PATH_PAIR), rr.all_distances(IP, xb, xq, orc.PATH_BLAS)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_model_edges():
    xb, xq = _data(9, 50, 5, 4)
    lims, D, I = rr.flat_range(L2, xb, xq, np.inf)
    assert lims.tolist() == [0, 50, 100, 150, 200] and np.array_equal(I, np.tile(np.arange(50), 4))
    for metric in (L2, IP):
        lims, D, I = rr.flat_range(metric, xb, xq, np.nan)
        assert lims.tolist() == [0] * 5 and D.size == 0 and I.size == 0
    lims, D, I = rr.flat_range(L2, xb, xq, 0.0)
    assert lims[-1] == 0  # strict: the three queries equal to rows are at distance 0
    dis = rr.flat_matrix(L2, xb, xq)
    v = np.sort(dis.ravel())[20]
    assert rr.flat_range(L2, xb, xq, v)[0][-1] == int((dis < v).sum()) < int((dis <= v).sum())  # the value itself is excluded
    keep = np.arange(50) % 3 == 0
    lims, D, I = rr.flat_range(L2, xb, xq, np.inf, labels=np.arange(50) * 7 + 3, keep=keep)
    assert lims[-1] == 4 * keep.sum() and set(I.tolist()) == set((np.arange(50)[keep] * 7 + 3).tolist())
