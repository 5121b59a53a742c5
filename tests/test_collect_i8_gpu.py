"""The d <= 128 coarse filter on its int8 store (csrc/flat_collect.hip "int8 store"): the same labels and distances, bit
for bit, as the bf16 store (option cl_i8 = 0) and as the exact f32 kernel -- L2 and inner product, with an IDSelector, lists of 32, 100
and 1000 entries, outlier rows -- and a store whose columns the int8 grid cannot hold stays on bf16."""

import numpy as np
import pytest

L2, IP = 1, 0
KERNEL = "flat_bf16_collect_kernel"


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss

    return mi355_faiss


def _index(mf, d, metric, xb, prefilter, i8=1):
    ix = mf.index_factory(d, "Flat", metric)
    ix.set_option("prefilter", prefilter)
    ix.set_option("cl_i8", i8)
    for i0 in range(0, len(xb), 1 << 16):
        ix.add(xb[i0 : i0 + (1 << 16)])
    return ix


def _same(a, b):
    (D1, I1), (D2, I2) = a, b
    return np.array_equal(I1, I2) and np.array_equal(D1.view(np.uint32), D2.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_i8_store_equals_bf16_store_and_exact_kernel(mf, metric):
    rs = np.random.RandomState(7 + metric)
    nb, nq, k = 1_000_000, 2000, 10
    xb = rs.rand(nb, 128).astype(np.float32)
    xq = rs.rand(nq, 128).astype(np.float32)
    i8 = _index(mf, 128, metric, xb, 2, 1)
    r8 = i8.search(xq, k)
    assert i8.last_kernel_info()["name"] == KERNEL
    assert i8.get_stat("cl_store_i8") == 1
    bf = _index(mf, 128, metric, xb, 2, 0)
    rb = bf.search(xq, k)
    assert bf.get_stat("cl_store_i8") == 0
    ex = _index(mf, 128, metric, xb, 0)
    re = ex.search(xq, k)
    assert _same(r8, rb), "int8 store differs from the bf16 store"
    assert _same(r8, re), "int8 store differs from the exact f32 kernel"
    # the option switches the same index between the stores
    i8.set_option("cl_i8", 0)
    assert _same(i8.search(xq, k), re) and i8.get_stat("cl_store_i8") == 0
    i8.set_option("cl_i8", 1)
    assert _same(i8.search(xq, k), re) and i8.get_stat("cl_store_i8") == 1


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("k", [32, 100, 1000])
def test_i8_store_lists_and_selector(mf, metric, k):
    rs = np.random.RandomState(100 + k + metric)
    nb, nq = 400_000, 600
    xb = rs.rand(nb, 128).astype(np.float32)
    xq = rs.rand(nq, 128).astype(np.float32)
    i8 = _index(mf, 128, metric, xb, 2, 1)
    ex = _index(mf, 128, metric, xb, 0)
    r8 = i8.search(xq, k)
    assert i8.get_stat("cl_store_i8") == 1
    assert _same(r8, ex.search(xq, k))
    ids = np.arange(0, nb, 3, dtype=np.int64)  # an IDSelector: every third row
    r8s = i8.search(xq, k, sel=("batch", ids))
    assert _same(r8s, ex.search(xq, k, sel=("batch", ids)))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_i8_store_outlier_rows(mf, metric):
    """rows of 100 x the usual norm are kept out of the int8 store too (zero row, beta_int = INT_MIN: never a candidate through the scan, never in a
    maximum) and reach every query's candidates through the appended list; uniform rows, so that the int8 store IS chosen"""
    rs = np.random.RandomState(31 + metric)
    nb, nq, k = 300_000, 400, 10
    xb = rs.rand(nb, 128).astype(np.float32)
    out_rows = [777, 150_000, 299_999]
    xb[out_rows] *= 100.0
    xq = rs.rand(nq, 128).astype(np.float32)
    xq[:3] = xb[out_rows] * 1.001  # queries that sit on the outliers (they clamp: a wide E of their own, still exact)
    i8 = _index(mf, 128, metric, xb, 2, 1)
    r8 = i8.search(xq, k)
    assert i8.get_stat("flat_outlier_rows") == 3
    assert i8.get_stat("cl_store_i8") == 1
    if metric == L2:
        assert [int(r8[1][j][0]) for j in range(3)] == out_rows
    ex = _index(mf, 128, metric, xb, 0)
    assert _same(r8, ex.search(xq, k))
    bf = _index(mf, 128, metric, xb, 2, 0)
    assert _same(r8, bf.search(xq, k))


@pytest.mark.gpu
def test_spiky_columns_keep_the_bf16_store(mf):
    rs = np.random.RandomState(5)
    nb, nq, k = 300_000, 300, 10
    xb = rs.rand(nb, 128).astype(np.float32)
    xb[:, 17] *= 4000.0  # one column spans 4000 x the others: the int8 grid of the store would drown the other 127
    xq = rs.rand(nq, 128).astype(np.float32)
    xq[:, 17] *= 4000.0
    cl = _index(mf, 128, L2, xb, 2, 1)
    r = cl.search(xq, k)
    assert cl.get_stat("cl_store_i8") == 0
    ex = _index(mf, 128, L2, xb, 0)
    assert _same(r, ex.search(xq, k))
