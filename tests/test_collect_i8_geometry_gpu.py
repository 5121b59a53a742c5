"""The int8 instances of the d <= 128 coarse filter have a geometry of their own (csrc/flat_collect.hip: workgroups per CU, row splits,
staged blocks): whatever it is, the int8 store returns the labels and the distance bits of the exact f32 kernel (prefilter 0) -- L2 and
inner product -- for row counts that end inside every position of a staged block and of a tile, with an IDSelector, with lists of 32,
100 and 1000 entries, and with outlier rows in the last staged block.  Every case asserts the store and the kernel that served it, so
that none passes on another path."""

import numpy as np
import pytest

L2, IP = 1, 0
KERNEL = "flat_bf16_collect_kernel"
BASE = 262_144  # the smallest Flat index the int8 store serves
TAILS = [0, 1, 31, 33, 63, 65, 127, 129, 255]
NQ = 300


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss

    return mi355_faiss


@pytest.fixture(scope="module")
def data():
    rs = np.random.RandomState(2024)
    xb = rs.rand(BASE + 256, 128).astype(np.float32)
    xq = rs.rand(NQ, 128).astype(np.float32)
    return xb, xq


def _index(mf, metric, xb, prefilter):
    ix = mf.index_factory(128, "Flat", metric)
    ix.set_option("prefilter", prefilter)
    ix.set_option("cl_i8", 1)
    for i0 in range(0, len(xb), 1 << 16):
        ix.add(xb[i0 : i0 + (1 << 16)])
    return ix


def _same(a, b):
    (D1, I1), (D2, I2) = a, b
    return np.array_equal(I1, I2) and np.array_equal(D1.view(np.uint32), D2.view(np.uint32))


def _search_i8(ix, xq, k, **kw):
    r = ix.search(xq, k, **kw)
    assert ix.last_kernel_info()["name"] == KERNEL
    assert ix.get_stat("cl_store_i8") == 1
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("tail", TAILS)
def test_row_counts_ending_inside_a_staged_block(mf, data, metric, tail):
    xb, xq = data
    xb = xb[: BASE + tail]
    # sixteen queries sit on rows spread over the tail, so that the rows behind the last full block decide results
    n = len(xb)
    rows = np.unique(np.linspace(n - max(tail, 1), n - 1, 16).astype(np.int64))
    xq = xq.copy()
    xq[: len(rows)] = xb[rows]
    i8 = _index(mf, metric, xb, 2)
    ex = _index(mf, metric, xb, 0)
    r8 = _search_i8(i8, xq, 10)
    re = ex.search(xq, 10)
    assert ex.last_kernel_info()["name"] != KERNEL
    if metric == L2:
        assert [int(r8[1][j][0]) for j in range(len(rows))] == [int(r) for r in rows]
    assert _same(r8, re), "int8 store differs from the exact f32 kernel at N = %d" % n


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_selector_every_third_row(mf, data, metric):
    xb, xq = data
    xb = xb[: BASE + 129]
    i8 = _index(mf, metric, xb, 2)
    ex = _index(mf, metric, xb, 0)
    ids = np.arange(0, len(xb), 3, dtype=np.int64)
    r8 = _search_i8(i8, xq, 10, sel=("batch", ids))
    assert _same(r8, ex.search(xq, 10, sel=("batch", ids)))
    assert np.all(r8[1] % 3 == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("k", [32, 100, 1000])
def test_longer_lists(mf, data, metric, k):
    xb, xq = data
    xb = xb[: BASE + 65]
    i8 = _index(mf, metric, xb, 2)
    ex = _index(mf, metric, xb, 0)
    assert _same(_search_i8(i8, xq, k), ex.search(xq, k))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_outlier_rows_in_the_last_staged_block(mf, data, metric):
    xb, xq = data
    xb = xb[: BASE + 129].copy()
    n = len(xb)
    out_rows = [n - 128, n - 70, n - 1]  # rows of 100 x the usual norm: kept out of the int8 store, appended to every query's candidates
    xb[out_rows] *= 100.0
    xq = xq.copy()
    xq[:3] = xb[out_rows] * 1.001
    i8 = _index(mf, metric, xb, 2)
    ex = _index(mf, metric, xb, 0)
    r8 = _search_i8(i8, xq, 10)
    assert i8.get_stat("flat_outlier_rows") == 3
    if metric == L2:
        assert [int(r8[1][j][0]) for j in range(3)] == out_rows
    assert _same(r8, ex.search(xq, 10))
