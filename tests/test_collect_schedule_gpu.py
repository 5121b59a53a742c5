"""The d <= 128 coarse-filter scan is a persistent kernel that pulls (row range, query block) items from eight queues (csrc/flat_collect.hip,
csrc/flat_collect.h): whatever the plan, the labels and the distance bits are those of the exact f32 kernel (prefilter 0).  The cases make
every workgroup loop over several items with queues of uneven length (so that workgroups take from other queues), launch fewer items than
slots, end the store in a range of a single partial stage or of two or three stages under many query blocks, run the other instances of the kernel (IDSelector, 32 classes with the
publish-only pre-pass, lists of 100 and 1000 with frozen bounds) and search one index twice with different batch sizes.  Every case asserts
the kernel and the store that served it."""

import numpy as np
import pytest

L2, IP = 1, 0
KERNEL = "flat_bf16_collect_kernel"
BASE = 262_144  # the smallest Flat index the int8 store serves
SLOTS_I8, SLOTS_BF16 = 768, 512  # resident workgroups of the scan: three / two per CU


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss

    return mi355_faiss


@pytest.fixture(scope="module")
def data():
    rs = np.random.RandomState(77)
    xb = rs.rand(BASE + 1024, 128).astype(np.float32)
    xq = rs.rand(61 * 512 + 17, 128).astype(np.float32)
    return xb, xq


def _index(mf, metric, xb, prefilter, i8=1):
    ix = mf.index_factory(128, "Flat", metric)
    ix.set_option("prefilter", prefilter)
    ix.set_option("cl_i8", i8)
    for i0 in range(0, len(xb), 1 << 16):
        ix.add(xb[i0 : i0 + (1 << 16)])
    return ix


def _same(a, b):
    (D1, I1), (D2, I2) = a, b
    return np.array_equal(I1, I2) and np.array_equal(D1.view(np.uint32), D2.view(np.uint32))


def _search(ix, xq, k, i8=1, **kw):
    r = ix.search(xq, k, **kw)
    assert ix.last_kernel_info()["name"] == KERNEL
    assert ix.get_stat("cl_store_i8") == i8
    return r


def _exact(mf, metric, xb, xq, k, **kw):
    ex = _index(mf, metric, xb, 0)
    r = ex.search(xq, k, **kw)
    assert ex.last_kernel_info()["name"] != KERNEL
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_more_items_than_slots_int8(mf, data, metric):
    xb, xq = data
    xb, xq = xb[: BASE + 77], xq[:16000]
    ix = _index(mf, metric, xb, 2)
    r = _search(ix, xq, 10)
    grid, items, ranges = ix.last_kernel_info()["grid"], ix.get_stat("cl_scan_items"), ix.get_stat("cl_scan_ranges")
    assert grid == SLOTS_I8 and items > grid, (grid, items)
    assert items == ranges * 32 and ranges % 8 != 0, (items, ranges)  # uneven queues: some workgroups take from another XCD's queue
    assert _same(r, _exact(mf, metric, xb, xq, 10))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_more_items_than_slots_bf16_store(mf, data, metric):
    xb, xq = data
    xb = xb[: 100_000 + 33]
    ix = _index(mf, metric, xb, 2, i8=0)
    r = _search(ix, xq, 10, i8=0)
    grid, items = ix.last_kernel_info()["grid"], ix.get_stat("cl_scan_items")
    assert grid == SLOTS_BF16 and items > grid and items % 62 == 0, (grid, items)  # 61 x 512 + 17 queries: 62 query blocks, the last of 17
    assert _same(r, _exact(mf, metric, xb, xq, 10))


@pytest.mark.gpu
def test_fewer_items_than_slots(mf, data):
    xb, xq = data
    xb, xq = xb[: BASE + 1], xq[:300]
    ix = _index(mf, L2, xb, 2)
    r = _search(ix, xq, 10)
    grid, items = ix.last_kernel_info()["grid"], ix.get_stat("cl_scan_items")
    assert 0 < items < SLOTS_I8 and grid == items, (grid, items)
    assert _same(r, _exact(mf, L2, xb, xq, 10))


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [1, 63, 65, 127, 129])
def test_last_range_is_a_partial_stage(mf, data, tail):
    # the taper ends in ranges of 512 rows (csrc/flat_collect.h CL_TAPER_FLOOR_ROWS) and 262 144 is a multiple of it: the rows behind it are
    # a range of their own -- one partial stage, or (129) a stage and one row; sixteen queries sit on them, as in the geometry test
    xb, xq = data
    xb = xb[: BASE + tail]
    n = len(xb)
    rows = np.unique(np.linspace(n - tail, n - 1, 16).astype(np.int64))
    xq = xq[:300].copy()
    xq[: len(rows)] = xb[rows]
    ix = _index(mf, L2, xb, 2)
    r = _search(ix, xq, 10)
    assert ix.get_stat("cl_scan_ranges") == BASE // 512 + 1
    assert [int(r[1][j][0]) for j in range(len(rows))] == [int(v) for v in rows]
    assert _same(r, _exact(mf, L2, xb, xq, 10))


@pytest.mark.gpu
@pytest.mark.parametrize("tail,last", [(129, 1), (257, 129), (385, 257)])
def test_short_last_range_with_many_query_blocks(mf, data, tail, last):
    # 32 query blocks: 206 ranges, the last one of `last` rows -- one stage (each of its 32 items ends before its successor is known: the
    # cold start), two or three (each takes its successor in its first stage, handed over warm by the item before it: the hand-over words
    # alternate, so a wave that reads its successor late never sees the following take).  Queries of every query block sit on those rows.
    xb, xq = data
    xb, xq = xb[: BASE + tail], xq[:16000]
    n = len(xb)
    xq = xq.copy()
    xq[100::512] = xb[np.linspace(n - last, n - 1, 32).astype(np.int64)]
    ix = _index(mf, L2, xb, 2)
    r = _search(ix, xq, 10)
    assert ix.get_stat("cl_scan_ranges") == 206 and ix.get_stat("cl_scan_items") == 206 * 32 > ix.last_kernel_info()["grid"]
    assert _same(r, _exact(mf, L2, xb, xq, 10))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_selector_every_third_row(mf, data, metric):
    xb, xq = data
    xb, xq = xb[: BASE + 77], xq[:16000]
    ids = np.arange(0, len(xb), 3, dtype=np.int64)
    ix = _index(mf, metric, xb, 2)
    r = _search(ix, xq, 10, sel=("batch", ids))
    assert ix.get_stat("cl_scan_items") > ix.last_kernel_info()["grid"]
    assert np.all(r[1] % 3 == 0)
    assert _same(r, _exact(mf, metric, xb, xq, 10, sel=("batch", ids)))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [32, 100, 1000])
def test_longer_lists(mf, data, k):
    # 32: 32 row classes and the publish-only pre-pass on the same kernel; 100: 128 classes; 1000: frozen bounds from a pass of their own
    xb, xq = data
    xb, xq = xb[: BASE + 77], xq[: 16000 if k < 1000 else 2048]
    ix = _index(mf, L2, xb, 2)
    r = _search(ix, xq, k)
    assert ix.get_stat("cl_scan_items") > ix.last_kernel_info()["grid"]
    assert _same(r, _exact(mf, L2, xb, xq, k))


@pytest.mark.gpu
def test_same_index_twice(mf, data):
    xb, xq = data
    xb = xb[: BASE + 77]
    ix = _index(mf, L2, xb, 2)
    ex = _index(mf, L2, xb, 0)
    plans = []
    for nq in (16000, 700, 16000):  # the cursors are zero again after every launch; the plan follows the batch
        r = _search(ix, xq[:nq], 10)
        plans.append((ix.last_kernel_info()["grid"], ix.get_stat("cl_scan_items")))
        assert _same(r, ex.search(xq[:nq], 10)), nq
    assert plans[0] == plans[2] and plans[0] != plans[1], plans
