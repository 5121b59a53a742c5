"""IVF<n>,PQ<M> / IDMap,IVF<n>,PQ<M> on the device against the CPU model of tests/ivfpq_reference.py: every comparison is bitwise
(labels array_equal, distances as uint32).  Where training is not under test both sides use the same coarse centroids and codebooks
through the setters, so a k-means mismatch cannot mask a scan bug."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ivfpq_reference as ivr
import pq_reference as pqr
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


def _index(d, desc, metric, cent, cb):
    ix = _mf().index_factory(d, desc, metric)
    assert not ix.is_trained
    ix.ivf_set_centroids(cent)
    assert not ix.is_trained  # trained once both the centroids and the codebooks are present
    ix.pq_set_centroids(cb)
    assert ix.is_trained
    return ix


def _lists_equal(ix, lists, what):
    for l, (ids_l, codes_l) in enumerate(lists):
        assert ix.ivfpq_list_size(l) == ids_l.size, f"{what}: list {l} holds {ix.ivfpq_list_size(l)} rows, the model {ids_l.size}"
        ids, codes = ix.ivfpq_list(l)
        assert np.array_equal(ids, ids_l), f"{what}: ids of list {l}"
        assert np.array_equal(codes, codes_l), f"{what}: codes of list {l}"


def _circle(nlist, d):
    """centroids far apart under both metrics: radius 100 on a circle in the first two dimensions (rows and queries within 0.5 of one)"""
    t = 2.0 * np.pi * np.arange(nlist) / nlist
    c = np.zeros((nlist, d), dtype=np.float32)
    c[:, 0], c[:, 1] = 100.0 * np.cos(t), 100.0 * np.sin(t)
    return c


def _near(rng, cent, counts):
    """counts[l] points within 0.5 of centroid l, shuffled -> (points, list of every point)"""
    of = np.repeat(np.arange(len(counts)), counts)
    of = of[rng.permutation(of.size)]
    return (cent[of] + rng.uniform(-0.5, 0.5, size=(of.size, cent.shape[1]))).astype(np.float32), of


# ------------------------------------------------------------------------------------------------ training
TRAIN_SHAPES = [(8, 2, 4), (12, 4, 3), (64, 4, 16)]


@functools.lru_cache(maxsize=None)
def _trained(d, M, nlist, metric):
    rng = np.random.default_rng(100 * d + M + metric)
    x = rng.standard_normal((2000, d)).astype(np.float32)
    x[rng.integers(0, 2000, 100)] = x[rng.integers(0, 2000, 100)]  # repeated rows: equal distances inside the k-means
    cent, cb = ivr.train(x, nlist, M, metric)
    for a in (x, cent, cb):
        a.setflags(write=False)
    return x, cent, cb


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,M,nlist", TRAIN_SHAPES)
def test_train_gives_the_reference_centroids_and_codebooks(d, M, nlist, metric):
    mf = _mf()
    x, cent, cb = _trained(d, M, nlist, metric)
    oiv = orc.Index(d, f"IVF{nlist},Flat", metric)
    oiv.train(x)
    ix = mf.index_factory(d, f"IVF{nlist},PQ{M}", metric)
    assert ix.kind == mf.KIND_IVFPQ == 6 and not ix.is_trained and ix.pq_info() == (M, 8) and ix.nlist == nlist
    if (d, M) == (8, 2):
        ix.train(x[:1000])  # ntotal == 0: training again is accepted
    ix.train(x)
    assert ix.is_trained and ix.quantizer.ntotal == nlist
    assert np.array_equal(ix.ivf_centroids().view(np.uint32), oiv.ivf_centroids().view(np.uint32))
    assert np.array_equal(ix.pq_centroids().view(np.uint32), cb.view(np.uint32))
    ix.add(x[:5])
    with pytest.raises(mf.FaissException, match="only possible while it is empty"):
        ix.train(x)


def test_train_needs_enough_rows_and_add_needs_training():
    mf = _mf()
    x, _, _ = _trained(8, 2, 4, L2)
    for desc in ("IVF300,PQ2", "IVF4,PQ2", "IDMap,IVF4,PQ2"):
        ix = mf.index_factory(8, desc, L2)
        with pytest.raises(mf.FaissException, match="at least as large as number of clusters"):
            ix.train(x[:299] if "300" in desc else x[:255])  # n < nlist / n < 256
        assert not ix.is_trained
        with pytest.raises(mf.FaissException, match="is_trained"):
            ix.add_with_ids(x[:10], np.arange(10)) if desc.startswith("IDMap") else ix.add(x[:10])
        assert ix.ntotal == 0


# ------------------------------------------------------------------------------------------------ add
@pytest.mark.parametrize("how", ["add", "add_with_ids", "IDMap"])
def test_lists_equal_the_reference_whatever_the_batches(how):
    rng = np.random.default_rng(17)
    d, M, nlist, n = 12, 4, 5, 6000
    cent = (3.0 * rng.standard_normal((nlist, d))).astype(np.float32)
    cb = pqr.synthetic_codebooks(rng, M, d // M)
    of = rng.integers(0, nlist, n)
    xb = (cent[of] + rng.standard_normal((n, d))).astype(np.float32)
    xb[:300] = cent[of[:300]] + cb[:, rng.integers(0, 256, 300)].transpose(1, 0, 2).reshape(300, d)  # centroid + codebook entries (also duplicated ones)
    ids = None if how == "add" else rng.permutation(10 * n)[:n].astype(np.int64)
    ix = _index(d, "IDMap,IVF5,PQ4" if how == "IDMap" else "IVF5,PQ4", L2, cent, cb)
    i0 = 0
    for m in (1, 19, 20, 1000, n - 1040):  # batch independence, growth of the code store
        ix.add(xb[i0 : i0 + m]) if ids is None else ix.add_with_ids(xb[i0 : i0 + m], ids[i0 : i0 + m])
        i0 += m
    assert ix.ntotal == n
    # under IDMap the lists hold the sequence numbers and id_map carries the external ids
    lists = ivr.build_lists(L2, cent, cb, xb, ids=None if how == "IDMap" else ids)
    _lists_equal(ix, lists, how)
    D, I = ix.search(xb[:7], 10, nprobe=3)
    _same(D, I, *ivr.search(L2, cent, cb, lists, xb[:7], 10, 3, id_map=ids if how == "IDMap" else None), how)


# ------------------------------------------------------------------------------------------------ search
SEARCH_SHAPES = [(1, 8), (3, 4), (16, 4), (33, 1), (64, 2), (128, 1), (2, 80)]  # float4 x3, float2 x2, scalar; (2, 80): v does not fit LDS


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("M,dsub", SEARCH_SHAPES)
def test_search_equals_the_model(metric, M, dsub):
    mf = _mf()
    d, nlist = M * dsub, 32
    rng = np.random.default_rng(1000 * M + dsub + metric)
    cb = (0.3 * pqr.synthetic_codebooks(rng, M, dsub)).astype(np.float32)
    cent = _circle(nlist, d)
    ix = _index(d, f"IVF{nlist},PQ{M}", metric, cent, cb)
    Q, R = ix.get_stat("ivfpq_pair_block"), ix.get_stat("ivfpq_rows_per_workgroup")
    assert 1 <= Q <= 32 and R >= 64
    # an empty trained index: every slot is padding
    D, I = ix.search(cent[:3], 5, nprobe=4)
    assert (I == -1).all() and (D == (ivr.FLT_MAX if metric == L2 else -ivr.FLT_MAX)).all()
    # skewed lists: R, R - 1, R + 1 and > 2 R rows, lists below 64 rows, empty ones (the segment edges do not depend on the table layout:
    # beyond M = 32, where the CPU model's encoder is slow, R and R - 1 shrink to lists around one wavefront)
    edge = [R, R - 1] if M <= 32 else [64, 65]
    counts = np.concatenate([[edge[0], 0, edge[1], 37, R + 1, 0, 2 * R + 3, 63], rng.integers(0, 150, nlist - 8)])
    counts[[9, 20]] = 0
    xb, of = _near(rng, cent, counts)
    dst, src = rng.integers(0, xb.shape[0], 2000), rng.integers(0, xb.shape[0], 2000)
    same = of[dst] == of[src]
    xb[dst[same]] = xb[src[same]]  # duplicate rows inside a list -> tied sums
    ix.add(xb[:5000])
    ix.add(xb[5000:])
    lists = ivr.build_lists(metric, cent, cb, xb)
    assert [i.size for i, _ in lists][:8] == counts[:8].tolist()
    _lists_equal(ix, lists, "skewed lists")
    # queries: lists 0 / 2 / 4 / 6 are the nearest of Q - 1 / Q / Q + 1 / 2 Q + 1 of them, a short and two empty lists of one each
    qcounts = np.zeros(nlist, dtype=np.int64)
    qcounts[[0, 2, 4, 6, 3, 1, 9]] = [Q - 1, Q, Q + 1, 2 * Q + 1, 1, 1, 1]
    xq, _ = _near(rng, cent, qcounts)
    dis = ivr.all_pair_distances(metric, cent, cb, lists, xq)
    ks = [1, 10, 100, 1000, 2048]
    for i, nprobe in enumerate([1, 2, 3, 4, 9, nlist, nlist + 7]):
        k = ks[i % 5]
        D, I = ix.search(xq, k, nprobe=nprobe)
        _same(D, I, *ivr.select(metric, ivr.probes(metric, cent, xq, nprobe), lists, dis, k), f"M={M} nprobe={nprobe} k={k}")
    assert ix.last_kernel_info()["name"] == "ivfpq_scan_kernel"
    # k beyond the probed rows, one query, the index's own nprobe (1)
    D, I = ix.search(xq, 2048, nprobe=1)
    Dr, Ir = ivr.select(metric, ivr.probes(metric, cent, xq, 1), lists, dis, 2048)
    _same(D, I, Dr, Ir, f"M={M} nprobe=1 k=2048")
    assert (I == -1).any() and (I[I >= 0] < xb.shape[0]).all()
    for nprobe, k in ((3, 10), (0, 100)):
        D, I = ix.search(xq[:1], k, nprobe=nprobe)
        _same(D, I, *ivr.select(metric, ivr.probes(metric, cent, xq[:1], max(nprobe, 1)), lists, [v if v is None else v[:1] for v in dis], k),
              f"M={M} one query nprobe={nprobe}")


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nlist", [1, 5])
def test_few_lists(metric, nlist):
    rng = np.random.default_rng(40 + nlist + metric)
    d, M = 12, 3
    cb = (0.3 * pqr.synthetic_codebooks(rng, M, d // M)).astype(np.float32)
    cent = _circle(nlist, d)
    ix = _index(d, f"IVF{nlist},PQ{M}x8", metric, cent, cb)
    xb, _ = _near(rng, cent, [700] if nlist == 1 else [0, 70, 900, 0, 11])
    xq, _ = _near(rng, cent, [9] * nlist)
    ix.add(xb)
    lists = ivr.build_lists(metric, cent, cb, xb)
    _lists_equal(ix, lists, f"nlist={nlist}")
    dis = ivr.all_pair_distances(metric, cent, cb, lists, xq)
    for nprobe, k in ((1, 10), (2, 100), (nlist, 1000), (nlist + 7, 1)):
        D, I = ix.search(xq, k, nprobe=nprobe)
        _same(D, I, *ivr.select(metric, ivr.probes(metric, cent, xq, nprobe), lists, dis, k), f"nlist={nlist} nprobe={nprobe} k={k}")


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("metric", [L2, IP])
def test_integer_lattice_ties_follow_probe_rank_then_position(metric):
    rng = np.random.default_rng(50 + metric)
    d, M, nlist = 4, 2, 5
    j = np.arange(256)
    cb = np.empty((M, 256, 2), dtype=np.float32)
    cb[:, :, 0], cb[:, :, 1] = j // 16 - 8, j % 16 - 8  # all 256 points of [-8, 7]^2
    cent = np.array([[0, 0, 0, 0], [40, 3, 0, 1], [-2, 41, 5, 0], [1, -3, 43, 2], [-39, 2, -4, 44]], dtype=np.float32)
    of = rng.integers(0, nlist, 4000)
    xb = (cent[of] + rng.integers(-3, 4, size=(4000, d))).astype(np.float32)  # 7^4 residuals per list: many equal rows
    xb[3000:3500] = xb[2000:2500]
    xq = (cent[rng.integers(0, nlist, 40)] + rng.integers(-8, 8, size=(40, d))).astype(np.float32)
    # (the probe order is the quantiser's business, pinned elsewhere: keep the queries whose coarse values -- exact integers -- are distinct)
    coarse = xq.astype(np.int64) @ cent.astype(np.int64).T if metric == IP else ((xq[:, None, :] - cent[None]).astype(np.int64) ** 2).sum(-1)
    xq = xq[[len(set(row)) == nlist for row in coarse.tolist()]][:21]
    assert xq.shape[0] >= 10
    ix = _index(d, "IVF5,PQ2", metric, cent, cb)
    ix.add(xb)
    lists = ivr.build_lists(metric, cent, cb, xb)
    _lists_equal(ix, lists, "lattice")
    dis = ivr.all_pair_distances(metric, cent, cb, lists, xq)
    assert all(np.array_equal(v, np.rint(v)) for v in dis)  # exact sums
    for nprobe in (1, 3, 5):
        P = ivr.probes(metric, cent, xq, nprobe)
        for k in (1, 10, 100):
            D, I = ix.search(xq, k, nprobe=nprobe)
            _same(D, I, *ivr.select(metric, P, lists, dis, k), f"lattice nprobe={nprobe} k={k}")
            if k > 1:
                assert (D[:, -1] == D[:, -2]).any()  # the boundary is tied for some query


# ------------------------------------------------------------------------------------------------ overflow, Python-written images
def test_sums_improving_with_position_overflow_the_buckets_and_are_rescanned(tmp_path):
    """a list of more than 2 R rows whose codes are written through a file so that the sums DEcrease with the position: probed at
    rank 0 by one query and at rank 1 by another"""
    mf = _mf()
    R = _index(2, "IVF3,PQ2", L2, np.zeros((3, 2), dtype=np.float32), np.zeros((2, 256, 1), dtype=np.float32)).get_stat("ivfpq_rows_per_workgroup")
    n = 2 * R + 5
    assert n <= 65536
    cb = np.zeros((2, 256, 1), dtype=np.float32)
    cb[0, :, 0] = 256.0 * np.arange(256)
    cb[1, :, 0] = np.arange(256)
    cent = np.array([[0, 0], [40000, 0], [-3000, 0]], dtype=np.float32)
    v = np.arange(n)[::-1]  # position p holds the point (256 (v // 256), v % 256), v = n - 1 - p: closer to the left with every position
    lists = [(np.arange(n, dtype=np.int64) + 100, np.stack([v // 256, v % 256], axis=1).astype(np.uint8)),
             (np.array([7, 8, 9], dtype=np.int64), np.array([[0, 1], [0, 2], [0, 1]], dtype=np.uint8)),
             (np.array([1, 2, 3], dtype=np.int64), np.array([[1, 1], [0, 0], [1, 1]], dtype=np.uint8))]
    path = str(tmp_path / "descending.index")
    ivr.write_ivfpq(path, 2, L2, cent, cb, lists, nprobe=2)
    ix = mf.read_index(path)
    assert ix.kind == mf.KIND_IVFPQ and ix.ntotal == n + 6 and ix.is_trained
    _lists_equal(ix, lists, "Python-written image")
    xq = np.array([[-10, 0], [-2000, 0], [39000, 7], [-10, 300]], dtype=np.float32)  # list 0 at rank 0, 1, 1 (worsening), 0
    assert ivr.probes(L2, cent, xq, 2).tolist() == [[0, 2], [2, 0], [1, 0], [0, 2]]
    for k in (1, 10, 1000):
        D, I = ix.search(xq, k)  # (the image's own nprobe: 2)
        _same(D, I, *ivr.search(L2, cent, cb, lists, xq, k, 2), f"descending sums k={k}")
        assert I[0, 0] == 100 + n - 1
        assert ix.get_stat("ivfpq_scan_rescans") > 0
    assert ix.get_stat("ivfpq_scan_launches") > ix.get_stat("ivfpq_scan_rescans")


# ------------------------------------------------------------------------------------------------ selectors
@pytest.mark.parametrize("metric", [L2, IP])
def test_selectors_bare_and_under_idmap(metric):
    rng = np.random.default_rng(60 + metric)
    d, M, nlist, n = 12, 4, 5, 3000
    cb = (0.3 * pqr.synthetic_codebooks(rng, M, d // M)).astype(np.float32)
    cent = _circle(nlist, d)
    xb, of = _near(rng, cent, [600] * nlist)
    xq, _ = _near(rng, cent, [3] * nlist)
    ids = rng.permutation(3 * n)[:n].astype(np.int64)
    lists_seq = ivr.build_lists(metric, cent, cb, xb)
    dis = ivr.all_pair_distances(metric, cent, cb, lists_seq, xq)
    P = ivr.probes(metric, cent, xq, 3)
    for how in ("bare", "IDMap"):
        ix = _index(d, "IVF5,PQ4" if how == "bare" else "IDMap,IVF5,PQ4", metric, cent, cb)
        ix.add_with_ids(xb, ids)
        lists = lists_seq if how == "IDMap" else [(ids[i], c) for i, c in lists_seq]  # bare: the lists store the ids themselves
        id_map = ids if how == "IDMap" else None
        _same(*ix.search(xq, 10, nprobe=3), *ivr.select(metric, P, lists, dis, 10, id_map=id_map), how + ", no selector")
        for keep in (ids % 3 == 0, of != 2):  # (of != 2: the selector empties a probed list)
            for k in (10, 1500):
                Dr, Ir = ivr.select(metric, P, lists, dis, k, id_map=id_map, keep_ids=ids[keep])
                _same(*ix.search(xq, k, nprobe=3, sel=("bitmap", bitmap_from_ids(ids, keep))), Dr, Ir, f"{how} bitmap k={k}")
                _same(*ix.search(xq, k, nprobe=3, sel=("batch", ids[keep])), Dr, Ir, f"{how} batch k={k}")
        D, I = ix.search(xq, 10, nprobe=5, sel=("batch", np.array([3 * n + 5], dtype=np.int64)))
        assert (I == -1).all() and (D == (ivr.FLT_MAX if metric == L2 else -ivr.FLT_MAX)).all()


# ------------------------------------------------------------------------------------------------ persistence, placement
@pytest.mark.parametrize("desc", ["IVF5,PQ4", "IDMap,IVF5,PQ4"])
def test_write_read_clone_and_refused_sharding(desc, tmp_path):
    mf = _mf()
    rng = np.random.default_rng(71)
    d, M, nlist, n = 12, 4, 5, 2500
    cb = (0.3 * pqr.synthetic_codebooks(rng, M, d // M)).astype(np.float32)
    cent = _circle(nlist, d)
    xb, _ = _near(rng, cent, [1000, 0, 1200, 300, 0])
    xq, _ = _near(rng, cent, [2] * nlist)
    wrapped = desc.startswith("IDMap")
    ids = rng.permutation(10 * n)[:n].astype(np.int64) if wrapped else None
    ix = _index(d, desc, IP, cent, cb)
    ix.add(xb) if ids is None else ix.add_with_ids(xb, ids)
    lists = ivr.build_lists(IP, cent, cb, xb)
    Dr, Ir = ivr.search(IP, cent, cb, lists, xq, 20, 3, id_map=ids)
    _same(*ix.search(xq, 20, nprobe=3), Dr, Ir, desc)
    # write -> the Python parser sees the model's lists; read_index gives equal lists and an equal search
    path = str(tmp_path / "a.index")
    mf.write_index(ix, path)
    img = ivr.parse_ivfpq(path)
    assert (img["d"], img["ntotal"], img["trained"], img["metric"], img["nlist"], img["nprobe"]) == (d, n, True, IP, nlist, 1)
    assert (img["by_residual"], img["code_size"], img["M"], img["nbits"]) == (1, M, M, 8)
    assert np.array_equal(img["centroids"].view(np.uint32), cent.view(np.uint32)) and np.array_equal(img["codebooks"].view(np.uint32), cb.view(np.uint32))
    for (ids_a, codes_a), (ids_b, codes_b) in zip(img["lists"], lists):
        assert np.array_equal(ids_a, ids_b) and np.array_equal(codes_a, codes_b)
    assert (img["id_map"] is None) if ids is None else np.array_equal(img["id_map"], ids)
    back = mf.read_index(path)
    assert back.ntotal == n and back.is_trained and back.pq_info() == (M, 8) and back.nlist == nlist
    _lists_equal(back, lists, desc + " after read_index")
    _same(*back.search(xq, 20, nprobe=3), Dr, Ir, desc + " after read_index")
    # a Python-written file loads and searches identically
    path2 = str(tmp_path / "b.index")
    ivr.write_ivfpq(path2, d, IP, cent, cb, lists, id_map=ids)
    _same(*mf.read_index(path2).search(xq, 20, nprobe=3), Dr, Ir, desc + " from a Python-written file")
    # what this path does not serve is refused on reading
    for kwargs, msg in ((dict(by_residual=0), "by_residual"), (dict(nbits=4), "8 bits per code only"), (dict(fourcc=b"IwQR"), "IwQR")):
        path3 = str(tmp_path / "refused.index")
        ivr.write_ivfpq(path3, d, IP, cent, cb, lists, **kwargs)
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
    assert not empty.is_trained and empty.ntotal == 0 and empty.pq_info() == (M, 8) and empty.nlist == nlist


def test_sharded_factory_is_refused():
    """env MVS_DEVICES at creation: a fresh process, as the variable is read when the index is made"""
    code = (
        "import sys; sys.path.insert(0, %r); import mi355_faiss as mf\n"
        "try:\n    mf.index_factory(8, 'IDMap,IVF4,PQ4', 1)\nexcept mf.FaissException as e:\n    print('REFUSED', e)\n"
    ) % os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, MVS_DEVICES="0,0"))
    assert out.returncode == 0, out.stderr
    assert "REFUSED" in out.stdout and "This index type is not implemented" in out.stdout


# ------------------------------------------------------------------------------------------------ factory, errors
def test_factory_strings_and_refusals():
    mf = _mf()
    for desc in ("IVF8,PQ4", "IVF8,PQ4x8", "IDMap,IVF8,PQ4", "IDMap2,IVF8,PQ4x8"):
        ix = mf.index_factory(8, desc, IP)
        inner = ix.index if desc.startswith("IDMap") else ix
        assert inner.kind == mf.KIND_IVFPQ and ix.pq_info() == (4, 8) and ix.nlist == 8 and not ix.is_trained
        assert inner.quantizer is not None and inner.quantizer.kind == mf.KIND_FLAT
    assert mf.index_factory(256, "IVF2,PQ128", L2).pq_info() == (128, 8)
    for desc, msg in (("IVF8,PQ4x4", "8 bits per code only"), ("IVF8,PQ256", "128"), ("IVF8_HNSW4,PQ4", "IVF8_HNSW4,PQ4"), ("OPQ4,IVF8,PQ4", "OPQ4")):
        with pytest.raises(mf.FaissException, match="This index type is not implemented on the MI355X path yet: .*" + msg):
            mf.index_factory(256 if "256" in desc else 8, desc, L2)
    with pytest.raises(mf.FaissException, match="multiple of the number of subquantizers"):
        mf.index_factory(8, "IVF8,PQ5", L2)
    with pytest.raises(mf.FaissException, match="metric type 2 is not implemented on the MI355X path"):
        mf.index_factory(8, "IVF8,PQ4", 2)
    rng = np.random.default_rng(3)
    ix = _index(8, "IVF2,PQ4", L2, _circle(2, 8), pqr.synthetic_codebooks(rng, 4, 2))
    x, _ = _near(rng, _circle(2, 8), [20, 20])
    ix.add(x)
    with pytest.raises(mf.FaissException, match="2048"):
        ix.search(x[:1], 2049)
    with pytest.raises(mf.FaissException, match="k > 0"):
        ix.search(x[:1], 0)
    with pytest.raises(mf.FaissException, match="not a PQ index"):
        ix.pq_codes()  # the codes of an IVFPQ index live in its lists
    with pytest.raises(mf.FaissException, match="not an IVFPQ index"):
        mf.index_factory(8, "IVF2,Flat", L2).ivfpq_list_size(0)


# ------------------------------------------------------------------------------------------------ cross-kind
@pytest.mark.parametrize("metric", [L2, IP])
def test_one_list_with_a_zero_centroid_is_the_pq_index(metric):
    mf = _mf()
    rng = np.random.default_rng(80 + metric)
    d, M = 32, 8
    cb = pqr.synthetic_codebooks(rng, M, d // M)
    xb = rng.standard_normal((3000, d)).astype(np.float32)
    xb[rng.integers(0, 3000, 400)] = xb[rng.integers(0, 3000, 400)]
    xq = rng.standard_normal((11, d)).astype(np.float32)
    a = _index(d, "IVF1,PQ8", metric, np.zeros((1, d), dtype=np.float32), cb)
    b = mf.index_factory(d, "PQ8", metric)
    b.pq_set_centroids(cb)
    a.add(xb)
    b.add(xb)
    assert np.array_equal(a.ivfpq_list(0)[1], b.pq_codes())
    for k in (1, 10, 1000):
        _same(*a.search(xq, k), *b.search(xq, k), f"IVF1,PQ8 vs PQ8 k={k}")


# ------------------------------------------------------------------------------------------------ the glue's cast (:675)
def test_idmap_ivfpq_through_the_cpp_glue_path():
    """boundary_driver ingest: chunked AddFunction from two threads (buffered: the index needs training), AddFinaliseFunction (train + add),
    then a search whose parameters come from innerCreateSearchParameters"""
    out = subprocess.run([DRIVER, "ingest", "3000", "8", "2", "IDMap,IVF4,PQ4"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ingest\tOK ntotal=3000" in out.stdout


def test_the_glue_casts_to_index_ivf_and_its_nprobe_reaches_the_search():
    out = subprocess.run([DRIVER, "ivfpq", "3000", "8"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ivfpq\tOK IndexIVF=1 IndexPQ=0 nlist=4 ntotal=3000" in out.stdout
