"""Shared by tests/test_merge_gpu.py and tests/test_copy_subset_gpu.py: parameters that need no training, rows, the comparison of a merged
index with its yardstick through every public entry point, and the CPU models' answer for every kind.  A helper module: nothing here is
collected."""
import functools

import numpy as np

import ivfpq_reference as ivr
import pq_reference as pqr
import sq_reference as sqr
from oracle import oracle as orc

L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
PAIRS = [(0, 5), (5, 0), (1, 40), (16, 17), (17, 16), (31, 33), (48, 1)]
COARSE_KERNEL = "flat_bf16_collect_kernel"


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def base_of(desc):
    return desc.split(",", 1)[1] if desc.startswith("IDMap") else desc


def is_ivf(desc):
    return base_of(desc).startswith("IVF")


def circle(nlist, d):
    """centroids far apart under both metrics: radius 100 on a circle in the first two dimensions"""
    t = 2.0 * np.pi * np.arange(nlist) / nlist
    c = np.zeros((nlist, d), dtype=np.float32)
    c[:, 0], c[:, 1] = 100.0 * np.cos(t), 100.0 * np.sin(t)
    return c


@functools.lru_cache(maxsize=None)
def params_of(base, d):
    """the trained state of a kind, without training: centroids, codebooks, range"""
    rng = np.random.default_rng(7 * d + len(base))
    p = {}
    if base.startswith("IVF"):
        p["cent"] = circle(int(base[3 : base.index(",")].split("_")[0]), d)
    if "PQ" in base:
        M = int(base[base.index("PQ") + 2 :])
        p["cb"] = (0.3 * pqr.synthetic_codebooks(rng, M, d // M)).astype(np.float32)
    if "SQ8" in base:
        lo = -0.6 if base.startswith("IVF") else -0.3
        p["sq"] = (np.full(d, lo, np.float32), (np.float32(1.2) + 0.01 * np.arange(d)).astype(np.float32))
    return p


def make(mf, desc, d, metric=L2, p=None):
    p = params_of(base_of(desc), d) if p is None else p
    ix = mf.index_factory(d, desc, metric)
    if "cent" in p:
        ix.ivf_set_centroids(p["cent"])
    if "cb" in p:
        ix.pq_set_centroids(p["cb"])
    if "sq" in p:
        ix.sq_set_trained(*p["sq"])
    assert ix.is_trained
    return ix


@functools.lru_cache(maxsize=None)
def rows_of(d, n, seed=0, lists=None):
    """n rows; about a tenth duplicated so that the order of ties shows.  lists: the list of every row (points within 0.5 of a centroid)"""
    rng = np.random.default_rng(1000 * d + 10 * n + seed)
    x = rng.random((n, d), dtype=np.float32) - np.float32(0.25)
    if lists is not None:
        x = (circle(4, d)[np.asarray(lists, dtype=np.int64)] + (x - np.float32(0.25))).astype(np.float32)
    if n >= 10:
        x[n // 2 :: 5][: n // 10] = x[: len(x[n // 2 :: 5][: n // 10])]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def queries_of(d, nq, ivf=False):
    rng = np.random.default_rng(977 * d + nq)
    xq = rng.random((nq, d), dtype=np.float32) - np.float32(0.25)
    if ivf:
        xq = (circle(4, d)[rng.integers(0, 4, nq)] + (xq - np.float32(0.25))).astype(np.float32)
    xq.setflags(write=False)
    return xq


def fill(ix, x, ids=None):
    if len(x) == 0:
        return
    if ids is None:
        ix.add(x)
    else:
        ix.add_with_ids(x, np.asarray(ids, dtype=np.int64))


def file_bytes(mf, ix, tmp_path, name):
    p = str(tmp_path / name)
    mf.write_index(ix, p)
    with open(p, "rb") as f:
        return f.read()


def lists_of(ix, desc):
    base = base_of(desc)
    if not is_ivf(desc) or base.endswith("Flat"):
        return None  # (IVF<n>,Flat: the lists are compared through the file image)
    get = ix.ivfpq_list if "PQ" in base else ix.ivfsq_list
    return [get(l) for l in range(4)]


def assert_indistinguishable(mf, a, b, desc, d, tmp_path, what, keys=None, nprobes=(0,)):
    """a (merged) against b (the yardstick) through every public entry point"""
    assert a.ntotal == b.ntotal, what
    n = a.ntotal
    for nq in (3, 25):  # FAISS's per-pair branch and its BLAS branch
        xq = queries_of(d, nq, is_ivf(desc))
        for k in (1, 5, n + 3):
            for nprobe in nprobes:
                Da, Ia = a.search(xq, k, nprobe=nprobe)
                Db, Ib = b.search(xq, k, nprobe=nprobe)
                assert np.array_equal(Ia, Ib), f"{what}: labels differ at nq {nq} k {k} nprobe {nprobe}"
                assert np.array_equal(u32(Da), u32(Db)), f"{what}: distances are not bit-equal at nq {nq} k {k} nprobe {nprobe}"
    if base_of(desc).endswith("Flat") and n > 0:
        xq = queries_of(d, 25, is_ivf(desc))
        radius = np.float32(np.median(b.search(xq, min(5, n), nprobe=4)[0][:, -1]))
        ga, gb = a.range_search(xq, radius, nprobe=4), b.range_search(xq, radius, nprobe=4)
        assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[2], gb[2]) and np.array_equal(u32(ga[1]), u32(gb[1])), f"{what}: range_search differs"
    if n > 0:
        if keys is None:
            assert np.array_equal(u32(a.reconstruct_n(0, n)), u32(b.reconstruct_n(0, n))), f"{what}: reconstruct_n differs"
        else:
            keys = np.unique(np.asarray(keys, dtype=np.int64))
            assert np.array_equal(u32(a.reconstruct_batch(keys)), u32(b.reconstruct_batch(keys))), f"{what}: reconstruct_batch differs"
    la, lb = lists_of(a, desc), lists_of(b, desc)
    if la is not None:
        for l in range(4):
            assert np.array_equal(la[l][0], lb[l][0]) and np.array_equal(la[l][1], lb[l][1]), f"{what}: list {l} differs"
    assert file_bytes(mf, a, tmp_path, "a.index") == file_bytes(mf, b, tmp_path, "b.index"), f"{what}: the bytes write_index produces differ"


def assert_emptied(mf, b, desc, d, what):
    assert b.ntotal == 0 and b.is_trained, what
    if desc.startswith("IDMap"):
        assert b.index.ntotal == 0, what
    D, I = b.search(queries_of(d, 3, is_ivf(desc)), 4, nprobe=4)
    assert (I == -1).all(), f"{what}: the emptied index still returns labels"


def model_search(desc, d, metric, x, stored, ext, xq, k, nprobe):
    """the CPU models' answer for an index that holds rows x with stored ids `stored` (None: the row numbers) under id map `ext`"""
    base = base_of(desc)
    p = params_of(base, d)
    if base == "Flat":
        return orc.flat_search(metric, x, xq, k, id_map=ext)
    if base.startswith("PQ"):
        return pqr.search(p["cb"], pqr.encode(p["cb"], x), xq, k, metric, labels=ext)
    if base == "SQ8":
        return sqr.sq_search(metric, *p["sq"], sqr.encode(*p["sq"], x), xq, k, labels=ext)
    if base.endswith("Flat"):
        o = orc.Index(d, desc, metric)
        o.ivf_set_centroids(p["cent"])
        if ext is not None:
            o.add_with_ids(x, ext)
        elif stored is not None:
            o.add_with_ids(x, stored)
        else:
            o.add(x)
        return o.search(xq, k, nprobe=nprobe)
    if "PQ" in base:
        lists = ivr.build_lists(metric, p["cent"], p["cb"], x, ids=stored)
        return ivr.search(metric, p["cent"], p["cb"], lists, xq, k, nprobe, id_map=ext)
    lists = sqr.build_lists(metric, p["cent"], *p["sq"], x, ids=stored)
    return sqr.ivf_search(metric, p["cent"], *p["sq"], lists, xq, k, nprobe, id_map=ext)


def assert_matches_model(a, desc, d, metric, x, stored, ext, what, nprobe=4):
    for nq in (3, 25):
        xq = queries_of(d, nq, is_ivf(desc))
        k = min(5, len(x))
        D, I = a.search(xq, k, nprobe=nprobe)
        Dm, Im = model_search(desc, d, metric, x, stored, ext, xq, k, nprobe)
        assert np.array_equal(I, Im), f"{what}: labels differ from the CPU model at nq {nq}"
        assert np.array_equal(u32(D), u32(Dm)), f"{what}: distances differ from the CPU model at nq {nq}"


