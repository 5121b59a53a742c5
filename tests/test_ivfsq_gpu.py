"""IVF<n>,SQ8 / IDMap,IVF<n>,SQ8 on the device against the CPU model of tests/sq_reference.py: every comparison of codes, labels and
distances is bitwise (labels array_equal, distances as uint32).  Where training is not under test both sides use the same coarse
centroids and range through the setters, so a k-means mismatch cannot mask a scan bug."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import sq_reference as sqr
from helpers import bitmap_from_ids
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "duckdb-faiss-ext_amd", "host", "boundary_driver")
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT


def _mf():
    import mi355_faiss as mf

    return mf


def _same(D, I, Dr, Ir, what):
    assert np.array_equal(I, Ir), f"{what}: labels differ in {(I != Ir).sum()} slots, first query {np.argwhere(I != Ir)[0][0]}"
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32)), f"{what}: distances differ in {(D != Dr).sum()} slots"


def _index(d, desc, metric, cent, vmin, vdiff):
    ix = _mf().index_factory(d, desc, metric)
    assert not ix.is_trained
    ix.ivf_set_centroids(cent)
    assert not ix.is_trained  # trained once both the centroids and the range are present
    ix.sq_set_trained(vmin, vdiff)
    assert ix.is_trained
    return ix


def _lists_equal(ix, lists, what):
    for l, (ids_l, codes_l) in enumerate(lists):
        assert ix.ivfsq_list_size(l) == ids_l.size, f"{what}: list {l} holds {ix.ivfsq_list_size(l)} rows, the model {ids_l.size}"
        ids, codes = ix.ivfsq_list(l)
        assert np.array_equal(ids, ids_l), f"{what}: ids of list {l}"
        assert np.array_equal(codes, codes_l), f"{what}: codes of list {l}"


def _circle(nlist, d):
    """centroids far apart under both metrics: radius 100 on a circle in the first two dimensions (d = 1: on a line, 200 apart)"""
    c = np.zeros((nlist, d), dtype=np.float32)
    if d == 1:
        c[:, 0] = 200.0 * np.arange(nlist) - 100.0 * (nlist - 1)
        return c
    t = 2.0 * np.pi * np.arange(nlist) / nlist
    c[:, 0], c[:, 1] = 100.0 * np.cos(t), 100.0 * np.sin(t)
    return c


def _near(rng, cent, counts):
    """counts[l] points within 0.5 of centroid l, shuffled -> (points, list of every point)"""
    of = np.repeat(np.arange(len(counts)), counts)
    of = of[rng.permutation(of.size)]
    return (cent[of] + rng.uniform(-0.5, 0.5, size=(of.size, cent.shape[1]))).astype(np.float32), of


def _range_of(metric, cent, x):
    of_row, _ = sqr.assign(metric, cent, x)
    return sqr.train_range(sqr.residuals(cent, x, of_row))


# ------------------------------------------------------------------------------------------------ training
@functools.lru_cache(maxsize=None)
def _trained(d, nlist, metric):
    rng = np.random.default_rng(100 * d + nlist + metric)
    x = rng.standard_normal((2000, d)).astype(np.float32)
    x[rng.integers(0, 2000, 100)] = x[rng.integers(0, 2000, 100)]  # repeated rows: equal distances inside the k-means
    x[:, d - 1] = 2.5  # a constant dimension of the ROWS is not one of the residuals
    cent, vmin, vdiff = sqr.ivf_train(x, nlist, metric)
    for a in (x, cent, vmin, vdiff):
        a.setflags(write=False)
    return x, cent, vmin, vdiff


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,nlist", [(8, 4), (12, 3), (64, 16)])
def test_train_gives_the_reference_centroids_and_the_range_of_the_residuals(d, nlist, metric):
    mf = _mf()
    x, cent, vmin, vdiff = _trained(d, nlist, metric)
    ix = mf.index_factory(d, f"IVF{nlist},SQ8", metric)
    assert ix.kind == mf.KIND_IVFSQ == 8 and not ix.is_trained and ix.nlist == nlist
    if d == 8:
        ix.train(x[:1000])  # ntotal == 0: training again is accepted
    ix.train(x)
    assert ix.is_trained and ix.quantizer.ntotal == nlist
    assert np.array_equal(ix.ivf_centroids().view(np.uint32), cent.view(np.uint32))
    gmin, gdiff = ix.sq_trained()
    assert (gmin == vmin).all() and (gdiff == vdiff).all()  # (values: the sign of a zero minimum is not specified)
    ix.add(x[:700])
    _lists_equal(ix, sqr.build_lists(metric, cent, vmin, vdiff, x[:700]), "after train")
    with pytest.raises(mf.FaissException, match="only possible while it is empty"):
        ix.train(x)
    with pytest.raises(mf.FaissException, match="only possible while it is empty"):
        ix.sq_set_trained(vmin, vdiff)


def test_train_needs_enough_rows_and_add_needs_training():
    mf = _mf()
    x, cent, vmin, vdiff = _trained(8, 4, L2)
    for desc in ("IVF300,SQ8", "IDMap,IVF300,SQ8"):
        ix = mf.index_factory(8, desc, L2)
        with pytest.raises(mf.FaissException, match="at least as large as number of clusters"):
            ix.train(x[:299])
        with pytest.raises(mf.FaissException):
            ix.train(x[:0])
        assert not ix.is_trained
        with pytest.raises(mf.FaissException, match="is_trained"):
            ix.add_with_ids(x[:10], np.arange(10)) if desc.startswith("IDMap") else ix.add(x[:10])
        assert ix.ntotal == 0
    # the range alone does not train the index; the centroids complete it (in either order, under IDMap too)
    for desc in ("IVF4,SQ8", "IDMap,IVF4,SQ8"):
        ix = mf.index_factory(8, desc, L2)
        ix.sq_set_trained(vmin, vdiff)
        assert not ix.is_trained
        with pytest.raises(mf.FaissException, match="is_trained"):
            ix.search(x[:1], 1)
        ix.ivf_set_centroids(cent)
        assert ix.is_trained and (ix.index if desc.startswith("IDMap") else ix).quantizer.ntotal == 4
        gmin, gdiff = ix.sq_trained()
        assert np.array_equal(gmin.view(np.uint32), vmin.view(np.uint32)) and np.array_equal(gdiff.view(np.uint32), vdiff.view(np.uint32))


# ------------------------------------------------------------------------------------------------ add
@pytest.mark.parametrize("how", ["add", "add_with_ids", "IDMap"])
def test_lists_equal_the_reference_whatever_the_batches(how):
    rng = np.random.default_rng(17)
    d, nlist, n = 12, 5, 6000
    cent = (3.0 * rng.standard_normal((nlist, d))).astype(np.float32)
    of = rng.integers(0, nlist, n)
    xb = (cent[of] + rng.standard_normal((n, d))).astype(np.float32)
    vmin, vdiff = _range_of(L2, cent, xb[:3000])  # trained on half of the rows: the others fall outside the range here and there
    vdiff[3] = 0.0  # a constant dimension
    xb[5000:5200] *= 3.0  # far outside
    ids = None if how == "add" else rng.permutation(10 * n)[:n].astype(np.int64)
    ix = _index(d, "IDMap,IVF5,SQ8" if how == "IDMap" else "IVF5,SQ8", L2, cent, vmin, vdiff)
    i0 = 0
    for m in (1, 2048, 19, 1001, n - 3069):  # batch independence, growth of the code store
        ix.add(xb[i0 : i0 + m]) if ids is None else ix.add_with_ids(xb[i0 : i0 + m], ids[i0 : i0 + m])
        i0 += m
    assert ix.ntotal == n
    # under IDMap the lists hold the sequence numbers and id_map carries the external ids
    lists = sqr.build_lists(L2, cent, vmin, vdiff, xb, ids=None if how == "IDMap" else ids)
    allc = np.concatenate([c for _, c in lists])
    assert (allc[:, 3] == 0).all() and (allc == 0).any() and (allc == 255).any()
    _lists_equal(ix, lists, how)
    D, I = ix.search(xb[:7], 10, nprobe=3)
    _same(D, I, *sqr.ivf_search(L2, cent, vmin, vdiff, lists, xb[:7], 10, 3, id_map=ids if how == "IDMap" else None), how)


# ------------------------------------------------------------------------------------------------ search
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [1, 5, 16, 17, 100, 128, 768, 1536])  # padding of the 16-byte words, every edge of the 32-component chunks
def test_search_equals_the_model(metric, d):
    nlist = 8
    rng = np.random.default_rng(1000 * d + metric)
    cent = _circle(nlist, d)
    # lists around the 1024-row blocks a workgroup stages, a wavefront, one row; empty ones
    counts = np.array([1023, 0, 1025, 37, 1024, 0, 63, 1])
    xb, of = _near(rng, cent, counts)
    dst, src = rng.integers(0, xb.shape[0], 800), rng.integers(0, xb.shape[0], 800)
    same = of[dst] == of[src]
    xb[dst[same]] = xb[src[same]]  # duplicate rows inside a list -> tied values
    vmin, vdiff = _range_of(metric, cent, xb)
    ix = _index(d, f"IVF{nlist},SQ8", metric, cent, vmin, vdiff)
    Q, R = ix.get_stat("sq_pair_block"), ix.get_stat("sq_rows_per_workgroup")
    assert 1 <= Q <= 32 and R >= 1024
    # an empty trained index: every slot is padding
    D, I = ix.search(cent[:3], 5, nprobe=4)
    assert (I == -1).all() and (D == (sqr.FLT_MAX if metric == L2 else -sqr.FLT_MAX)).all()
    ix.add(xb[:1500])
    ix.add(xb[1500:])
    lists = sqr.build_lists(metric, cent, vmin, vdiff, xb)
    if metric == L2 or d > 1:
        assert [i.size for i, _ in lists] == counts.tolist()
    _lists_equal(ix, lists, "skewed lists")
    # queries: lists 0 / 2 / 4 / 6 are the nearest of Q - 1 / Q / Q + 1 / 2 Q + 1 of them, a short and two empty lists of one each
    qcounts = np.zeros(nlist, dtype=np.int64)
    qcounts[[0, 2, 4, 6, 3, 1, 5]] = [Q - 1, Q, Q + 1, 2 * Q + 1, 1, 1, 1]
    xq, _ = _near(rng, cent, qcounts)
    dis = sqr.all_pair_distances(metric, cent, vmin, vdiff, lists, xq)
    ks = [1, 10, 100, 2048]
    for i, nprobe in enumerate([1, 3, nlist, nlist + 7, 2]):
        k = ks[i % 4]
        D, I = ix.search(xq, k, nprobe=nprobe)
        _same(D, I, *sqr.ivf_select(metric, sqr.probes(metric, cent, xq, nprobe), lists, dis, k), f"d={d} nprobe={nprobe} k={k}")
    assert ix.last_kernel_info()["name"] == "sq8_scan_kernel"
    # k beyond the probed rows, the index's own nprobe (1)
    D, I = ix.search(xq, 2048)
    _same(D, I, *sqr.ivf_select(metric, sqr.probes(metric, cent, xq, 1), lists, dis, 2048), f"d={d} nprobe=1 k=2048")
    assert (I == -1).any() and (I[I >= 0] < xb.shape[0]).all()
    D, I = ix.search(xq[:1], 10, nprobe=3)
    _same(D, I, *sqr.ivf_select(metric, sqr.probes(metric, cent, xq[:1], 3), lists, [v if v is None else v[:1] for v in dis], 10), f"d={d} one query")


@pytest.mark.parametrize("metric", [L2, IP])
def test_lists_around_the_rows_of_a_workgroup(metric):
    """lists of R - 1, R, R + 1 and 2 R + 3 rows: the segment edges of the scan and the windows of the selection"""
    nlist, d = 6, 5
    rng = np.random.default_rng(30 + metric)
    cent = _circle(nlist, d)
    R = _index(d, "IVF6,SQ8", metric, cent, np.zeros(d), np.ones(d)).get_stat("sq_rows_per_workgroup")
    counts = np.array([R, R - 1, 0, R + 1, 2 * R + 3, 40])
    assert counts.sum() <= 45000
    xb, _ = _near(rng, cent, counts)
    vmin, vdiff = _range_of(metric, cent, xb)
    ix = _index(d, "IVF6,SQ8", metric, cent, vmin, vdiff)
    ix.add(xb)
    lists = sqr.build_lists(metric, cent, vmin, vdiff, xb)
    assert [i.size for i, _ in lists] == counts.tolist()
    _lists_equal(ix, lists, "lists around R")
    xq, _ = _near(rng, cent, [3, 3, 1, 3, 3, 1])
    dis = sqr.all_pair_distances(metric, cent, vmin, vdiff, lists, xq)
    for nprobe, k in ((1, 10), (2, 2048), (3, 100), (6, 1000)):
        D, I = ix.search(xq, k, nprobe=nprobe)
        _same(D, I, *sqr.ivf_select(metric, sqr.probes(metric, cent, xq, nprobe), lists, dis, k), f"nprobe={nprobe} k={k}")


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nlist", [1, 5])
def test_few_lists(metric, nlist):
    rng = np.random.default_rng(40 + nlist + metric)
    d = 12
    cent = _circle(nlist, d)
    xb, _ = _near(rng, cent, [700] if nlist == 1 else [0, 70, 900, 0, 11])
    xq, _ = _near(rng, cent, [9] * nlist)
    vmin, vdiff = _range_of(metric, cent, xb)
    ix = _index(d, f"IVF{nlist},SQ8", metric, cent, vmin, vdiff)
    ix.add(xb)
    lists = sqr.build_lists(metric, cent, vmin, vdiff, xb)
    _lists_equal(ix, lists, f"nlist={nlist}")
    dis = sqr.all_pair_distances(metric, cent, vmin, vdiff, lists, xq)
    for nprobe, k in ((1, 10), (2, 100), (nlist, 1000), (nlist + 7, 1)):
        D, I = ix.search(xq, k, nprobe=nprobe)
        _same(D, I, *sqr.ivf_select(metric, sqr.probes(metric, cent, xq, nprobe), lists, dis, k), f"nlist={nlist} nprobe={nprobe} k={k}")


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("metric", [L2, IP])
def test_integer_lattice_ties_follow_probe_rank_then_position(metric):
    rng = np.random.default_rng(50 + metric)
    d, nlist = 4, 5
    vmin, vdiff = np.full(d, -0.5, dtype=np.float32), np.full(d, 255.0, dtype=np.float32)  # s = 1, a = 0: a code decodes to itself
    cent = np.array([[0, 0, 0, 0], [40, 3, 0, 1], [-2, 41, 5, 0], [1, -3, 43, 2], [-39, 2, -4, 44]], dtype=np.float32)
    of = rng.integers(0, nlist, 4000)
    xb = (cent[of] + rng.integers(0, 7, size=(4000, d))).astype(np.float32)  # 7^4 residuals per list: many equal rows
    xb[3000:3500] = xb[2000:2500]
    xq = (cent[rng.integers(0, nlist, 40)] + rng.integers(-4, 12, size=(40, d))).astype(np.float32)
    # (the probe order is the quantiser's business, pinned elsewhere: keep the queries whose coarse values -- exact integers -- are distinct)
    coarse = xq.astype(np.int64) @ cent.astype(np.int64).T if metric == IP else ((xq[:, None, :] - cent[None]).astype(np.int64) ** 2).sum(-1)
    xq = xq[[len(set(row)) == nlist for row in coarse.tolist()]][:21]
    assert xq.shape[0] >= 10
    ix = _index(d, "IVF5,SQ8", metric, cent, vmin, vdiff)
    ix.add(xb)
    lists = sqr.build_lists(metric, cent, vmin, vdiff, xb)
    assert all(np.array_equal(sqr.decode(vmin, vdiff, c), c.astype(np.float32)) for _, c in lists)
    _lists_equal(ix, lists, "lattice")
    dis = sqr.all_pair_distances(metric, cent, vmin, vdiff, lists, xq)
    assert all(np.array_equal(v, np.rint(v)) for v in dis if v is not None)  # exact values (inner product leaves the zero centroid's list empty)
    for nprobe in (1, 3, 5):
        P = sqr.probes(metric, cent, xq, nprobe)
        for k in (1, 10, 100):
            D, I = ix.search(xq, k, nprobe=nprobe)
            _same(D, I, *sqr.ivf_select(metric, P, lists, dis, k), f"lattice nprobe={nprobe} k={k}")
            if k > 1:
                assert (D[:, -1] == D[:, -2]).any()  # the boundary is tied for some query


# ------------------------------------------------------------------------------------------------ overflow, Python-written images
def test_values_improving_with_position_overflow_the_buckets_and_are_rescanned(tmp_path):
    """a list of more than 2 R rows whose codes are written through a file so that the distances DEcrease with the position: probed at
    rank 0 by some queries and at rank 1 / 2 by others"""
    mf = _mf()
    R = _index(2, "IVF3,SQ8", L2, np.zeros((3, 2), dtype=np.float32), np.zeros(2), np.ones(2)).get_stat("sq_rows_per_workgroup")
    n = 2 * R + 5
    assert n <= 65536
    # s = (256, 1), a = 0: the code (c0, c1) decodes to the point (256 c0, c1)
    vmin, vdiff = np.array([-128.0, -0.5], dtype=np.float32), np.array([256.0 * 255.0, 255.0], dtype=np.float32)
    cent = np.array([[0, 0], [40000, 0], [-3000, 0]], dtype=np.float32)
    v = np.arange(n)[::-1]  # position p holds the point (256 (v // 256), v % 256), v = n - 1 - p: closer to the left with every position
    lists = [(np.arange(n, dtype=np.int64) + 100, np.stack([v // 256, v % 256], axis=1).astype(np.uint8)),
             (np.array([7, 8, 9], dtype=np.int64), np.array([[0, 1], [0, 2], [0, 1]], dtype=np.uint8)),
             (np.array([1, 2, 3], dtype=np.int64), np.array([[1, 1], [0, 0], [1, 1]], dtype=np.uint8))]
    assert np.array_equal(sqr.decode(vmin, vdiff, lists[0][1]), np.stack([256.0 * (v // 256), v % 256], axis=1).astype(np.float32))
    path = str(tmp_path / "descending.index")
    sqr.write_ivfsq(path, 2, L2, cent, vmin, vdiff, lists, nprobe=2)
    ix = mf.read_index(path)
    assert ix.kind == mf.KIND_IVFSQ and ix.ntotal == n + 6 and ix.is_trained
    _lists_equal(ix, lists, "Python-written image")
    xq = np.array([[-10, 0], [-2000, 0], [39000, 7], [-10, 300]], dtype=np.float32)  # list 0 at rank 0, 1, 1 (worsening), 0
    assert sqr.probes(L2, cent, xq, 2).tolist() == [[0, 2], [2, 0], [1, 0], [0, 2]]
    dis = sqr.all_pair_distances(L2, cent, vmin, vdiff, lists, xq)
    for nprobe in (0, 3):  # (0: the image's own nprobe, 2; 3: list 0 inside a span of two ranks)
        for k in (1, 10, 1000):
            D, I = ix.search(xq, k, nprobe=nprobe)
            _same(D, I, *sqr.ivf_select(L2, sqr.probes(L2, cent, xq, nprobe or 2), lists, dis, k), f"descending values nprobe={nprobe} k={k}")
            assert I[0, 0] == 100 + n - 1
            assert ix.get_stat("sq_scan_rescans") > 0
            assert ix.get_stat("sq_scan_launches") > ix.get_stat("sq_scan_rescans")


# ------------------------------------------------------------------------------------------------ selectors
@pytest.mark.parametrize("metric", [L2, IP])
def test_selectors_bare_and_under_idmap(metric):
    rng = np.random.default_rng(60 + metric)
    d, nlist, n = 12, 5, 3000
    cent = _circle(nlist, d)
    xb, of = _near(rng, cent, [600] * nlist)
    xq, _ = _near(rng, cent, [3] * nlist)
    vmin, vdiff = _range_of(metric, cent, xb)
    ids = rng.permutation(3 * n)[:n].astype(np.int64)
    lists_seq = sqr.build_lists(metric, cent, vmin, vdiff, xb)
    dis = sqr.all_pair_distances(metric, cent, vmin, vdiff, lists_seq, xq)
    P = sqr.probes(metric, cent, xq, 3)
    for how in ("bare", "IDMap"):
        ix = _index(d, "IVF5,SQ8" if how == "bare" else "IDMap,IVF5,SQ8", metric, cent, vmin, vdiff)
        ix.add_with_ids(xb, ids)
        lists = lists_seq if how == "IDMap" else [(ids[i], c) for i, c in lists_seq]  # bare: the lists store the ids themselves
        id_map = ids if how == "IDMap" else None
        _same(*ix.search(xq, 10, nprobe=3), *sqr.ivf_select(metric, P, lists, dis, 10, id_map=id_map), how + ", no selector")
        for keep in (ids % 3 == 0, of != 2):  # (of != 2: the selector empties a probed list)
            for k in (10, 1500):
                Dr, Ir = sqr.ivf_select(metric, P, lists, dis, k, id_map=id_map, keep_ids=ids[keep])
                _same(*ix.search(xq, k, nprobe=3, sel=("bitmap", bitmap_from_ids(ids, keep))), Dr, Ir, f"{how} bitmap k={k}")
                _same(*ix.search(xq, k, nprobe=3, sel=("batch", ids[keep])), Dr, Ir, f"{how} batch k={k}")
        D, I = ix.search(xq, 10, nprobe=5, sel=("batch", np.array([3 * n + 5], dtype=np.int64)))
        assert (I == -1).all() and (D == (sqr.FLT_MAX if metric == L2 else -sqr.FLT_MAX)).all()


# ------------------------------------------------------------------------------------------------ persistence, placement
@pytest.mark.parametrize("desc", ["IVF5,SQ8", "IDMap,IVF5,SQ8"])
def test_write_read_clone_and_refused_sharding(desc, tmp_path):
    mf = _mf()
    rng = np.random.default_rng(71)
    d, nlist, n = 12, 5, 2500
    cent = _circle(nlist, d)
    xb, _ = _near(rng, cent, [1000, 0, 1200, 300, 0])
    xq, _ = _near(rng, cent, [2] * nlist)
    vmin, vdiff = _range_of(IP, cent, xb)
    wrapped = desc.startswith("IDMap")
    ids = rng.permutation(10 * n)[:n].astype(np.int64) if wrapped else None
    ix = _index(d, desc, IP, cent, vmin, vdiff)
    ix.add(xb) if ids is None else ix.add_with_ids(xb, ids)
    lists = sqr.build_lists(IP, cent, vmin, vdiff, xb)
    Dr, Ir = sqr.ivf_search(IP, cent, vmin, vdiff, lists, xq, 20, 3, id_map=ids)
    _same(*ix.search(xq, 20, nprobe=3), Dr, Ir, desc)
    # write -> the Python parser sees the model's lists; read_index gives equal lists and an equal search
    path = str(tmp_path / "a.index")
    mf.write_index(ix, path)
    img = sqr.parse_ivfsq(path)
    assert (img["d"], img["ntotal"], img["trained"], img["metric"], img["nlist"], img["nprobe"]) == (d, n, True, IP, nlist, 1)
    assert (img["qtype"], img["rangestat"], img["rangestat_arg"], img["sq_code_size"], img["code_size"], img["by_residual"]) == (0, 0, 0.0, d, d, 1)
    assert np.array_equal(img["centroids"].view(np.uint32), cent.view(np.uint32))
    assert np.array_equal(img["vmin"].view(np.uint32), vmin.view(np.uint32)) and np.array_equal(img["vdiff"].view(np.uint32), vdiff.view(np.uint32))
    for (ids_a, codes_a), (ids_b, codes_b) in zip(img["lists"], lists):
        assert np.array_equal(ids_a, ids_b) and np.array_equal(codes_a, codes_b)
    assert (img["id_map"] is None) if ids is None else np.array_equal(img["id_map"], ids)
    back = mf.read_index(path)
    assert back.ntotal == n and back.is_trained and back.nlist == nlist
    _lists_equal(back, lists, desc + " after read_index")
    _same(*back.search(xq, 20, nprobe=3), Dr, Ir, desc + " after read_index")
    # a Python-written file loads and searches identically
    path2 = str(tmp_path / "b.index")
    sqr.write_ivfsq(path2, d, IP, cent, vmin, vdiff, lists, id_map=ids)
    _same(*mf.read_index(path2).search(xq, 20, nprobe=3), Dr, Ir, desc + " from a Python-written file")
    # what this path does not serve is refused on reading
    for kwargs, msg in ((dict(qtype=1), "qtype = 1"), (dict(by_residual=0), "by_residual = 0"), (dict(code_size=2 * d), "code_size")):
        path3 = str(tmp_path / "refused.index")
        sqr.write_ivfsq(path3, d, IP, cent, vmin, vdiff, lists, **kwargs)
        with pytest.raises(mf.FaissException, match=msg):
            mf.read_index(path3)
    # clone_to_gpu(0): an independent copy; to_gpu(0) in place
    clone = ix.clone_to_gpu(0)
    extra, _ = _near(rng, cent, [2] * nlist)
    ix.add(extra) if ids is None else ix.add_with_ids(extra, np.arange(10) + 10**6)
    assert clone.ntotal == n and ix.ntotal == n + 10
    _same(*clone.search(xq, 20, nprobe=3), Dr, Ir, desc + " clone")
    clone.to_gpu(0)
    _same(*clone.search(xq, 20, nprobe=3), Dr, Ir, desc + " clone after to_gpu")
    # sharding is refused and leaves the index as it was
    before = clone.search(xq, 5, nprobe=2)
    with pytest.raises(mf.FaissException, match="This index type is not implemented"):
        clone.shard_to_gpus([0, 0])
    with pytest.raises(mf.FaissException, match="This index type is not implemented"):
        clone.clone_to_gpu(-1)
    if mf.device_count() >= 2:
        with pytest.raises(mf.FaissException, match="This index type is not implemented"):
            clone.shard_to_gpus([0, 1])
    assert clone.shard_info() is None and clone.ntotal == n
    _same(*clone.search(xq, 5, nprobe=2), *before, desc + " after the refused sharding")
    # an untrained, empty index round-trips too
    path4 = str(tmp_path / "c.index")
    mf.write_index(mf.index_factory(d, desc, L2), path4)
    empty = mf.read_index(path4)
    assert not empty.is_trained and empty.ntotal == 0 and empty.nlist == nlist


def test_sharded_factory_is_refused():
    """env MVS_DEVICES at creation: a fresh process, as the variable is read when the index is made"""
    code = (
        "import sys; sys.path.insert(0, %r); import mi355_faiss as mf\n"
        "try:\n    mf.index_factory(8, 'IDMap,IVF4,SQ8', 1)\nexcept mf.FaissException as e:\n    print('REFUSED', e)\n"
    ) % os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, MVS_DEVICES="0,0"))
    assert out.returncode == 0, out.stderr
    assert "REFUSED" in out.stdout and "This index type is not implemented" in out.stdout


# ------------------------------------------------------------------------------------------------ factory, errors
def test_factory_strings_and_refusals():
    mf = _mf()
    for desc in ("IVF8,SQ8", "IDMap,IVF8,SQ8", "IDMap2,IVF8,SQ8"):
        ix = mf.index_factory(8, desc, IP)
        inner = ix.index if desc.startswith("IDMap") else ix
        assert inner.kind == mf.KIND_IVFSQ and ix.nlist == 8 and not ix.is_trained
        assert inner.quantizer is not None and inner.quantizer.kind == mf.KIND_FLAT
    assert mf.index_factory(2048, "IVF2,SQ8", L2).d == 2048
    for desc, dd in (("IVF8,SQ4", 8), ("IVF8,SQ6", 8), ("IVF8,SQfp16", 8), ("IVF8,SQ8_direct", 8), ("IVF8,SQbf16", 8), ("IVF8_HNSW4,SQ8", 8),
                     ("IVF8,SQ8", 2049), ("IDMap,IVF8,SQ4", 8)):
        with pytest.raises(mf.FaissException, match="This index type is not implemented on the MI355X path yet: .*" + desc.split(",", 1)[-1 if desc.startswith("IDMap") else 0]):
            mf.index_factory(dd, desc, L2)
    with pytest.raises(mf.FaissException, match="metric type 2 is not implemented on the MI355X path"):
        mf.index_factory(8, "IVF8,SQ8", 2)
    rng = np.random.default_rng(3)
    x, _ = _near(rng, _circle(2, 8), [20, 20])
    ix = _index(8, "IVF2,SQ8", L2, _circle(2, 8), *_range_of(L2, _circle(2, 8), x))
    ix.add(x)
    with pytest.raises(mf.FaissException, match="2048"):
        ix.search(x[:1], 2049)
    with pytest.raises(mf.FaissException, match="k > 0"):
        ix.search(x[:1], 0)
    with pytest.raises(mf.FaissException, match="not an SQ8 index"):
        ix.sq_codes()  # the codes of the IVF kind live in its lists
    with pytest.raises(mf.FaissException, match="not an IVFSQ index"):
        mf.index_factory(8, "IVF2,Flat", L2).ivfsq_list_size(0)
    with pytest.raises(mf.FaissException, match="not an SQ index"):
        mf.index_factory(8, "IVF2,Flat", L2).sq_trained()


# ------------------------------------------------------------------------------------------------ cross-kind
@pytest.mark.parametrize("metric", [L2, IP])
def test_one_list_with_a_zero_centroid_is_the_sq8_index(metric):
    mf = _mf()
    rng = np.random.default_rng(80 + metric)
    d = 33
    xb = rng.standard_normal((3000, d)).astype(np.float32)
    xb[rng.integers(0, 3000, 400)] = xb[rng.integers(0, 3000, 400)]
    xq = rng.standard_normal((11, d)).astype(np.float32)
    vmin, vdiff = sqr.train_range(xb)
    a = _index(d, "IVF1,SQ8", metric, np.zeros((1, d), dtype=np.float32), vmin, vdiff)
    b = mf.index_factory(d, "SQ8", metric)
    b.sq_set_trained(vmin, vdiff)
    a.add(xb)
    b.add(xb)
    assert np.array_equal(a.ivfsq_list(0)[1], b.sq_codes())
    for k in (1, 10, 1000):
        _same(*a.search(xq, k), *b.search(xq, k), f"IVF1,SQ8 vs SQ8 k={k}")


# ------------------------------------------------------------------------------------------------ the glue's cast (:675)
def test_idmap_ivfsq_through_the_cpp_glue_path():
    """boundary_driver ingest: chunked AddFunction from two threads (buffered: the index needs training), AddFinaliseFunction (train + add),
    then a search whose parameters come from innerCreateSearchParameters"""
    out = subprocess.run([DRIVER, "ingest", "3000", "8", "2", "IDMap,IVF8,SQ8"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ingest\tOK ntotal=3000" in out.stdout
