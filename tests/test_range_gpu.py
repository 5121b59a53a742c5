"""Range search on the device (include/mi355_faiss.h "range search") against the CPU model of tests/range_reference.py:
lims and labels equal as integers, distances as bit patterns.  The shapes are the smallest that reach each edge: the branch switch at 20
queries, one and several 32-query wave blocks, a 256-row tile edge at (5, 257), d beyond 128 (the VALU formula mode), the stream overflow."""
import functools
import os
import subprocess

import numpy as np
import pytest

import range_reference as rr
from helpers import bitmap_from_ids
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

L2, IP = rr.L2, rr.IP
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (5, 257), (64, 1000), (128, 3000), (132, 700), (768, 520)]
NQS = [1, 19, 20, 33, 129]


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss as m

    assert m.device_count() >= 1
    return m


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"{what}: lims differ\n got {got[0][:12]}\n ref {want[0][:12]}"
    assert np.array_equal(got[2], want[2]), f"{what}: labels differ"
    assert np.array_equal(u32(got[1]), u32(want[1])), f"{what}: distances are not bit-exact"


@functools.lru_cache(maxsize=None)
def rows_of(d, n):
    rng = np.random.default_rng(1000 * d + n)
    xb = rng.random((n, d), dtype=np.float32) - np.float32(0.25)
    dup = np.arange(n // 2, n, 5)[: n // 10]  # about a tenth of the rows duplicated
    xb[dup] = xb[: dup.size]
    xb.setflags(write=False)
    return xb


@functools.lru_cache(maxsize=None)
def flat_case(metric, d, n, nq):
    """-> rows, queries, the model's distance matrix of the batch's branch (computed once, shared, read-only)"""
    xb = rows_of(d, n)
    rng = np.random.default_rng(77 * d + n + nq)
    xq = rng.random((nq, d), dtype=np.float32) - np.float32(0.25)
    for j, r in enumerate((0, n // 2, n - 1)[: min(3, nq)]):  # three queries equal to rows
        xq[j] = xb[r]
    dis = rr.flat_matrix(metric, xb, xq)
    xq.setflags(write=False)
    dis.setflags(write=False)
    return xb, xq, dis


def model_radii(dis):
    """the model's 1 % quantile, its median, and exactly one value that occurs in the matrix (strictness: that value is excluded)"""
    flat = np.sort(dis.ravel())
    return [np.float32(np.quantile(flat, 0.01)), np.float32(np.quantile(flat, 0.5)), flat[(flat.size * 3) // 10]]


@functools.lru_cache(maxsize=None)
def flat_index(metric, d, n):
    import mi355_faiss as m

    ix = m.index_factory(d, "Flat", metric)
    ix.add(rows_of(d, n))
    return ix


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("d,n", SHAPES)
@pytest.mark.parametrize("metric", [L2, IP])
def test_flat_matches_the_model(mf, metric, d, n, nq):
    xb, xq, dis = flat_case(metric, d, n, nq)
    ix = flat_index(metric, d, n)
    ix.set_option("range_mfma", 1)
    exact = model_radii(dis)[2]
    assert int((dis == exact).sum()) >= 1
    for radius in model_radii(dis):
        got = ix.range_search(xq, radius)
        assert_same(got, rr.select(metric, dis, radius), f"radius {radius!r}")
        name = ix.last_kernel_info()["name"]
        assert name == ("range_mfma_kernel" if nq >= 20 and d <= 128 else "range_pair_kernel"), name
    # the edges of the rule
    every, none = (np.inf, -np.inf) if metric == L2 else (-np.inf, np.inf)
    got = ix.range_search(xq, every)
    assert got[0][-1] == nq * n
    assert_same(got, rr.select(metric, dis, every), "every row")
    for radius in (none, np.nan) + ((0.0, -1.0) if metric == L2 else ()):
        lims, D, I = ix.range_search(xq, radius)
        assert lims.tolist() == [0] * (nq + 1) and D.size == 0 and I.size == 0, radius
    if nq >= 20:  # the VALU formula mode gives the MFMA kernel's bytes
        median = model_radii(dis)[1]
        a = ix.range_search(xq, median)
        ix.set_option("range_mfma", 0)
        b = ix.range_search(xq, median)
        ix.set_option("range_mfma", 1)
        assert ix.last_kernel_info()["name"] == "range_pair_kernel"
        assert_same(b, a, "range_mfma = 0 against 1")


@pytest.mark.parametrize("metric", [L2, IP])
def test_stream_overflow_is_rescanned_once(mf, metric):
    xb, xq, dis = flat_case(metric, 64, 1000, 33)
    median = model_radii(dis)[1]
    ix = mf.index_factory(64, "Flat", metric)
    ix.add(xb)
    auto = ix.range_search(xq, median)
    before = ix.get_stat("range_rescans")
    ix.set_option("range_stream_cap", 64)
    small = ix.range_search(xq, median)
    assert ix.get_stat("range_rescans") == before + 1
    assert_same(small, auto, "range_stream_cap = 64 against automatic")
    assert_same(small, rr.select(metric, dis, median))
    ix.set_option("range_stream_cap", 0)
    ix.range_search(xq, median)
    assert ix.get_stat("range_rescans") == before + 1


@pytest.mark.parametrize("nq", [5, 40])
@pytest.mark.parametrize("metric", [L2, IP])
def test_selectors_and_idmap(mf, metric, nq):
    d, n = 64, 1000
    xb, xq, _ = flat_case(metric, d, n, nq)
    keep = np.arange(n) % 3 == 0
    pair = rr.all_distances(metric, xb, xq, orc.PATH_PAIR)  # a selector sends the batch down the per-pair branch
    radius = np.float32(np.quantile(pair, 0.3))
    ix = flat_index(metric, d, n)
    for sel in (("bitmap", bitmap_from_ids(np.arange(n), keep)), ("batch", np.arange(n)[keep][::-1].copy())):
        assert_same(ix.range_search(xq, radius, sel=sel), rr.select(metric, pair, radius, keep=keep), sel[0])
    # IDMap: labels are id_map[row]; a selector tests the EXTERNAL id
    ids = 7 * np.arange(n, dtype=np.int64) + 3
    im = mf.index_factory(d, "IDMap,Flat", metric)
    im.add_with_ids(xb, ids)
    dis = rr.flat_matrix(metric, xb, xq)
    assert_same(im.range_search(xq, radius), rr.select(metric, dis, radius, labels=ids), "IDMap")
    for sel in (("bitmap", bitmap_from_ids(ids, keep)), ("batch", ids[keep])):
        assert_same(im.range_search(xq, radius, sel=sel), rr.select(metric, pair, radius, labels=ids, keep=keep), "IDMap " + sel[0])
    # a bitmap over ROW numbers keeps other rows under IDMap: bit `7 r + 3` is what is tested
    rowbits = bitmap_from_ids(np.arange(n), keep)
    ext_keep = np.array([(i >> 3) < rowbits.size and (rowbits[i >> 3] >> (i & 7)) & 1 for i in ids], dtype=bool)
    assert_same(im.range_search(xq, radius, sel=("bitmap", rowbits)), rr.select(metric, pair, radius, labels=ids, keep=ext_keep), "external id")


def test_staged_adds_empty_index_and_no_queries(mf):
    d = 16
    rng = np.random.default_rng(3)
    xb = rng.random((300, d), dtype=np.float32)
    xq = rng.random((25, d), dtype=np.float32)
    for desc in ("Flat", "IDMap,Flat"):
        ix = mf.index_factory(d, desc, L2)
        lims, D, I = ix.range_search(xq, 10.0)  # empty index: all lims are zero
        assert lims.tolist() == [0] * 26 and D.size == 0 and I.size == 0
        lims, D, I = ix.range_search(np.empty((0, d), np.float32), 10.0)  # no queries: lims = [0]
        assert lims.tolist() == [0] and D.size == 0 and I.size == 0
        ids = np.arange(300, dtype=np.int64) + 1000
        for r0 in range(0, 300, 100):  # small adds stay staged on the host until something reads the rows
            if desc == "Flat":
                ix.add(xb[r0 : r0 + 100])
            else:
                ix.add_with_ids(xb[r0 : r0 + 100], ids[r0 : r0 + 100])
            dis = rr.flat_matrix(L2, xb[: r0 + 100], xq)
            radius = np.float32(np.quantile(dis, 0.2))
            want = rr.select(L2, dis, radius, labels=None if desc == "Flat" else ids[: r0 + 100])
            assert_same(ix.range_search(xq, radius), want, f"{desc} after {r0 + 100} rows")
        lims, D, I = ix.range_search(np.empty((0, d), np.float32), 10.0)
        assert lims.tolist() == [0]


@pytest.mark.parametrize("desc", ["Flat", "IDMap,Flat"])
def test_placement_keeps_range_search_working(mf, desc):
    """to_gpu / clone_to_gpu around range searches: the hit stream and the sort buffers are per-device workspaces like every other one.
    (On one device to_gpu(0) is the no-op FAISS's call is there; with a second device the index really moves and its workspaces must not
    stay behind on the old one.)"""
    xb, xq, dis = flat_case(L2, 64, 1000, 33)
    ids = 7 * np.arange(1000, dtype=np.int64) + 3
    ix = mf.index_factory(64, desc, L2)
    if desc == "Flat":
        ix.add(xb)
    else:
        ix.add_with_ids(xb, ids)
    radius = model_radii(dis)[1]
    want = rr.select(L2, dis, radius, labels=None if desc == "Flat" else ids)
    assert_same(ix.range_search(xq, radius), want, "before")
    ix.to_gpu(0)
    assert_same(ix.range_search(xq, radius), want, "after to_gpu(0)")
    cl = ix.clone_to_gpu(0)
    assert_same(cl.range_search(xq, radius), want, "clone")
    if mf.device_count() >= 2:
        ix.to_gpu(1)
        assert ix.device == 1
        assert_same(ix.range_search(xq, radius), want, "after to_gpu(1)")
        ix.to_gpu(0)
        assert_same(ix.range_search(xq, radius), want, "back on device 0")


# ---- IVF
IVF_D, IVF_N = 32, 2000


@functools.lru_cache(maxsize=None)
def ivf_data():
    rng = np.random.default_rng(8)
    xb = rng.random((IVF_N, IVF_D), dtype=np.float32)
    cent = rng.random((8, IVF_D), dtype=np.float32)
    cent[6], cent[7] = -50.0, -100.0  # far from every row under both metrics: two lists stay empty
    xq = rng.random((40, IVF_D), dtype=np.float32)
    xq[0], xq[1] = xb[5], xb[1999]
    for a in (xb, cent, xq):
        a.setflags(write=False)
    return xb, cent, xq


@pytest.mark.parametrize("nq", [3, 40])
@pytest.mark.parametrize("idmap", [False, True])
@pytest.mark.parametrize("metric", [L2, IP])
def test_ivf_matches_the_model(mf, metric, idmap, nq):
    xb, cent, xq = ivf_data()
    xq = xq[:nq]
    ids = 7 * np.arange(IVF_N, dtype=np.int64) + 3
    g = mf.index_factory(IVF_D, "IDMap,IVF8,Flat" if idmap else "IVF8,Flat", metric)
    g.ivf_set_centroids(cent)
    if idmap:
        g.add_with_ids(xb, ids)
    else:
        g.add(xb)
    lists = rr.build_lists(metric, cent, xb)
    sizes = [len(l[0]) for l in lists]
    assert sizes[6] == 0 and sizes[7] == 0 and max(sizes) > 256, sizes
    allp = np.concatenate([rr.all_distances(metric, rows, xq, orc.PATH_PAIR).ravel() for _, rows in lists if len(rows)])
    radius = np.float32(np.quantile(allp, 0.3))
    for nprobe in (1, 3, 50):  # (50: beyond nlist -- clamped; the empty lists are probed too)
        P = rr.probes(metric, cent, xq, nprobe)
        want = rr.ivf_range(metric, lists, P, xq, radius, id_map=ids if idmap else None)
        got = g.range_search(xq, radius, nprobe=nprobe)
        assert_same(got, want, f"nprobe {nprobe}")
        assert g.last_kernel_info()["name"] == "range_pair_kernel"
    assert want[0][-1] > nq  # (the radius admits something)
    # nprobe 0: the index's own (1)
    assert_same(g.range_search(xq, radius), rr.ivf_range(metric, lists, rr.probes(metric, cent, xq, 1), xq, radius, id_map=ids if idmap else None))
    # selector keeping every third id (the external one under IDMap)
    lab = ids if idmap else np.arange(IVF_N, dtype=np.int64)
    keep_ids = lab[::3]
    P = rr.probes(metric, cent, xq, 3)
    want = rr.ivf_range(metric, lists, P, xq, radius, id_map=ids if idmap else None, keep_ids=set(keep_ids.tolist()))
    assert_same(g.range_search(xq, radius, nprobe=3, sel=("batch", keep_ids)), want, "batch selector")
    assert_same(g.range_search(xq, radius, nprobe=3, sel=("bitmap", bitmap_from_ids(lab, np.arange(IVF_N) % 3 == 0))), want, "bitmap selector")
    # the edges
    lims, D, I = g.range_search(xq, np.nan, nprobe=3)
    assert lims.tolist() == [0] * (nq + 1) and D.size == 0
    every = np.inf if metric == L2 else -np.inf
    assert_same(g.range_search(xq, every, nprobe=50), rr.ivf_range(metric, lists, rr.probes(metric, cent, xq, 50), xq, every, id_map=ids if idmap else None))
    assert g.range_search(xq, every, nprobe=50)[0][-1] == nq * IVF_N
    g.set_option("range_stream_cap", 64)
    before = g.get_stat("range_rescans")
    assert_same(g.range_search(xq, radius, nprobe=3, sel=("batch", keep_ids)), want, "overflow")
    assert g.get_stat("range_rescans") == before + 1


def test_ivf_repeated_ids_and_empty_index(mf):
    xb, cent, xq = ivf_data()
    g = mf.index_factory(IVF_D, "IVF8,Flat", L2)
    g.ivf_set_centroids(cent)
    lims, D, I = g.range_search(xq, 100.0, nprobe=8)  # trained but empty
    assert lims.tolist() == [0] * 41 and D.size == 0
    assert g.range_search(np.empty((0, IVF_D), np.float32), 1.0)[0].tolist() == [0]
    ids = np.arange(IVF_N, dtype=np.int64) % 500
    g.add_with_ids(xb, ids)
    lists = rr.build_lists(L2, cent, xb, ids)
    radius = np.float32(4.0)
    want = rr.ivf_range(L2, lists, rr.probes(L2, cent, xq, 4), xq, radius)
    assert want[0][-1] > 40
    assert_same(g.range_search(xq, radius, nprobe=4), want, "repeated ids")


@pytest.mark.parametrize("metric", [L2, IP])
def test_ivf_with_hnsw_quantiser(mf, metric):
    xb, _, xq = ivf_data()
    desc = "IVF16_HNSW8,Flat"
    o = orc.Index(IVF_D, desc, metric)
    g = mf.index_factory(IVF_D, desc, metric)
    g.set_option("hnsw_build_waves", 1)  # reaches the quantiser: the single-thread graph = the oracle's
    o.train(xb)
    g.train(xb)
    assert np.array_equal(u32(g.ivf_centroids()), u32(o.ivf_centroids()))
    o.add(xb)
    g.add(xb)
    lists = [o.ivf_list(l) for l in range(16)]
    _, P = g.quantizer.search(xq, 5, efSearch=64)  # the device's own probes: graph probes are not the Flat ones
    allp = np.concatenate([rr.all_distances(metric, rows, xq, orc.PATH_PAIR).ravel() for _, rows in lists if len(rows)])
    radius = np.float32(np.quantile(allp, 0.3))
    want = rr.ivf_range(metric, lists, P, xq, radius)
    assert want[0][-1] > 40
    assert_same(g.range_search(xq, radius, nprobe=5, efSearch=64), want, desc)


# ---- refusals
@pytest.mark.parametrize("desc", ["HNSW16", "PQ4", "SQ8", "IVF4,PQ2", "IVF4,SQ8", "SQ8,RFlat", "IDMap,PQ4"])
def test_other_kinds_refuse(mf, desc):
    ix = mf.index_factory(8, desc, L2)
    with pytest.raises(mf.FaissException, match="range search not implemented"):
        ix.range_search(np.zeros((2, 8), np.float32), 1.0)


def test_extra_metric_sharded_and_untrained_refuse(mf):
    x = np.random.default_rng(0).random((64, 8), dtype=np.float32)
    l1 = mf.index_factory(8, "Flat", 2)  # METRIC_L1
    l1.add(x)
    with pytest.raises(mf.FaissException, match="range search not implemented"):
        l1.range_search(x[:2], 1.0)
    sh = mf.index_factory(8, "Flat", L2)
    sh.add(x)
    assert sh.range_search(x[:2], 0.5)[0][-1] >= 2
    sh.shard_to_gpus([0, 0])
    with pytest.raises(mf.FaissException, match="range search not implemented"):
        sh.range_search(x[:2], 0.5)
    ivf = mf.index_factory(8, "IVF4,Flat", L2)
    assert not ivf.is_trained
    with pytest.raises(mf.FaissException, match="is_trained"):
        ivf.range_search(x[:2], 0.5)


# ---- the faiss:: classes: RangeSearchResult through the adaptor, checked against search inside the driver
@pytest.mark.parametrize("desc", ["IDMap,Flat", "IVF8,Flat"])
def test_boundary_driver_range(desc):
    drv = os.path.join(ROOT, "duckdb-faiss-ext_amd", "host", "boundary_driver")
    assert os.path.exists(drv), "build() makes host/boundary_driver"
    p = subprocess.run([drv, "range", "3000", "64", "40", desc], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    line = [l for l in p.stdout.splitlines() if l.startswith("RANGE OK")]
    assert line and int(line[0].split()[2]) > 0, p.stdout
