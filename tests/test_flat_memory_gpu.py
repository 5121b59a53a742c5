"""What a Flat index holds on the device between searches (csrc/dev_mem.h; csrc/index.h "the stores derived lazily from the rows"): the
stores are built, dropped, rebuilt, grown with their converted prefix kept and dropped again -- every search bit for bit the CPU oracle's --
and when the index is freed, statistic device_bytes_live, read through an index that stays alive, is back where it started: nothing leaks.

The Flat case is d = 32 with 262 400 rows: the int8 store and the outlier list start at 262 144 rows, so this is one 256-row block beyond
that threshold.  The IVF cases are about the quantiser (the counter sees the lists' own allocations too, so `live() == before` covers
them as well; tests/test_kind_memory_gpu.py is about those): IVF64, and IVF256, the smallest the bf16 coarse quantiser
(csrc/coarse_bf16.hip) serves."""

import gc

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss

    return mi355_faiss


@pytest.fixture
def live(mf):
    """reads device_bytes_live through a keeper index that outlives the index under test"""
    gc.collect()  # (garbage of earlier tests that holds an index goes now, not between two readings)
    keeper = mf.index_factory(8, "Flat", L2)
    return lambda: keeper.get_stat("device_bytes_live")


def _check(ix, metric, xb, xq, k, what):
    D, I = ix.search(xq, k)
    Do, Io = orc.flat_search(metric, xb, xq, k)
    assert np.array_equal(I, Io), what + ": labels differ from the oracle"
    assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), what + ": distances differ from the oracle"


@pytest.mark.parametrize("metric", [L2, IP])
def test_flat_stores_rebuild_grow_and_leave_nothing_behind(mf, live, metric):
    d, nq, k = 32, 256, 10
    rs = np.random.RandomState(41 + metric)
    xa = rs.rand(262_400, d).astype(np.float32)
    xb = rs.rand(290_000, d).astype(np.float32)
    xq = rs.rand(nq, d).astype(np.float32)
    before = live()
    ix = mf.index_factory(d, "Flat", metric)
    ix.add(xa)  # (one call: the row store holds exactly these rows, so the 20 000 below outgrow it)
    _check(ix, metric, xa, xq, k, "first build")
    assert ix.get_stat("cl_store_i8") == 1
    assert live() > before
    # the row store grows under stores that are built: they grow too, their converted prefix kept
    ix.add(xb[:20_000])
    _check(ix, metric, np.concatenate([xa, xb[:20_000]]), xq, k, "stores grown with the row store")
    assert ix.get_stat("cl_store_i8") == 1
    # every row goes, which drops what is derived from the rows as FlatIndex::reset() does (the C ABI has no reset for this kind);
    # 270 000 new rows: rebuilt after a drop
    assert ix.remove_ids(("batch", np.arange(ix.ntotal, dtype=np.int64))) == 282_400
    assert ix.ntotal == 0
    for i0 in range(0, 270_000, 1 << 16):
        ix.add(xb[i0 : min(i0 + (1 << 16), 270_000)])
    _check(ix, metric, xb[:270_000], xq, k, "rebuilt after a drop")
    assert ix.get_stat("cl_store_i8") == 1
    # 20 000 more: only they are converted
    ix.add(xb[270_000:])
    _check(ix, metric, xb, xq, k, "20 000 rows behind the converted ones")
    gone = rs.choice(290_000, 1000, replace=False).astype(np.int64)
    assert ix.remove_ids(("batch", gone)) == 1000
    _check(ix, metric, np.delete(xb, gone, axis=0), xq, k, "after remove_ids")
    del ix
    assert live() == before


@pytest.mark.parametrize("metric,nlist", [(L2, 64), (IP, 64), (L2, 256)])
def test_ivf_quantiser_leaves_nothing_behind(mf, live, metric, nlist):
    d, nb, nq, k, nprobe = 64, 20_000, 64, 10, 8
    xb = orc.synth_clustered(nb, d, 51, n_centers=nlist, sigma=0.15)
    xq = orc.synth_clustered(nq, d, 52, n_centers=nlist, sigma=0.15)
    desc = "IVF%d,Flat" % nlist
    o = orc.Index(d, desc, metric)
    o.train(xb)
    o.add(xb)
    Do, Io = o.search(xq, k, nprobe=nprobe)
    before = live()
    g = mf.index_factory(d, desc, metric)
    g.train(xb)  # (k-means: the quantiser is emptied and filled once per iteration, its coarse store built again each time)
    g.ivf_set_centroids(o.ivf_centroids())  # FlatIndex::reset() on a quantiser whose stores exist; the oracle's centroids from here on
    g.set_option("ivf_mfma", 0)  # (the scanner's arithmetic for inner product too, as tests/test_ivf_gpu.py compares it)
    g.add(xb)
    D, I = g.search(xq, k, nprobe=nprobe)
    assert np.array_equal(I, Io) and np.array_equal(D.view(np.uint32), Do.view(np.uint32))
    if nlist == 256:
        assert g.get_stat("coarse_bf16_queries") > 0  # (the quantiser did run on its bf16 coarse store)
    assert live() > before
    del g
    assert live() == before


def test_bf16x3_store_grows_and_leaves_nothing_behind(mf, live):
    """the bf16 hi/lo store of csrc/flat_bf16.hip (option prefilter = 1; d = 64: a shape that kernel serves, which d = 32 is not)"""
    d, k = 64, 10
    rs = np.random.RandomState(61)
    xb = rs.rand(9000, d).astype(np.float32)
    xq = rs.rand(64, d).astype(np.float32)
    before = live()
    ix = mf.index_factory(d, "Flat", L2)
    ix.set_option("prefilter", 1)
    ix.add(xb[:5000])  # (one call: exactly 5000 rows of room)
    _check(ix, L2, xb[:5000], xq, k, "first build")
    assert ix.last_kernel_info()["name"] == "flat_bf16x3_kernel"
    ix.add(xb[5000:])
    _check(ix, L2, xb, xq, k, "grown")
    assert ix.last_kernel_info()["name"] == "flat_bf16x3_kernel"
    del ix
    assert live() == before
