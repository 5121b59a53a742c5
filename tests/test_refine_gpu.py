"""<base>,RFlat / IDMap,<base>,RFlat on the device against the CPU model of tests/refine_reference.py: every comparison of labels and
distances is bitwise (labels array_equal, distances as uint32).  Codebooks, centroids and ranges are set through the accessors of the
base handle, so no k-means stands between the model and the kernels under test."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pq_reference as pqr
import refine_reference as rfr
import sq_reference as sqr
from helpers import bitmap_from_ids
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "duckdb-faiss-ext_amd", "host", "boundary_driver")
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
NOT_YET = "This index type is not implemented on the MI355X path yet"


def _mf():
    import mi355_faiss as mf

    return mf


def _same(D, I, Dr, Ir, what):
    assert np.array_equal(I, Ir), f"{what}: labels differ in {(I != Ir).sum()} slots, first query {np.argwhere(I != Ir)[0][0]}"
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32)), f"{what}: distances differ in {(D != Dr).sum()} slots"


def _desc(base, nlist, M):
    return {"PQ": f"PQ{M}", "IVFPQ": f"IVF{nlist},PQ{M}", "SQ": "SQ8", "IVFSQ": f"IVF{nlist},SQ8"}[base]


def _pair(base, d, metric, x, rng, nlist=4, M=None, idmap=False, suffix=",RFlat", prefix="IDMap,"):
    """-> (device index, model) with the same base parameters, both still empty; x: the rows that will be added (the range comes from them)"""
    mf = _mf()
    ix = mf.index_factory(d, (prefix if idmap else "") + _desc(base, nlist, M) + suffix, metric)
    assert not ix.is_trained
    b = ix.refine_base
    assert b is not None and ix.refine_store.kind == mf.KIND_FLAT
    assert b.kind == {"PQ": mf.KIND_PQ, "IVFPQ": mf.KIND_IVFPQ, "SQ": mf.KIND_SQ, "IVFSQ": mf.KIND_IVFSQ}[base]
    cent = cb = vmin = vdiff = None
    if base in ("IVFPQ", "IVFSQ"):
        cent = x[rng.permutation(len(x))[:nlist]].copy()
        b.ivf_set_centroids(cent)
    if base in ("PQ", "IVFPQ"):
        cb = pqr.synthetic_codebooks(rng, M, d // M)
        b.pq_set_centroids(cb)
    if base == "SQ":
        vmin, vdiff = sqr.train_range(x)
    if base == "IVFSQ":
        of_row, _ = sqr.assign(metric, cent, x)
        vmin, vdiff = sqr.train_range(sqr.residuals(cent, x, of_row))
    if vmin is not None:
        b.sq_set_trained(vmin, vdiff)
    assert b.is_trained and ix.is_trained  # (the wrappers see what was set behind their back)
    return ix, rfr.Model(base, metric, d, cent=cent, cb=cb, vmin=vmin, vdiff=vdiff)


def _like(m, M=None, prefix=""):
    """an empty device index with the model's base parameters"""
    ix = _mf().index_factory(m.d, prefix + _desc(m.base, 0 if m.cent is None else len(m.cent), M) + ",RFlat", m.metric)
    b = ix.refine_base
    if m.cent is not None:
        b.ivf_set_centroids(m.cent)
    if m.cb is not None:
        b.pq_set_centroids(m.cb)
    if m.vmin is not None:
        b.sq_set_trained(m.vmin, m.vdiff)
    assert ix.is_trained
    return ix


def _filled(base, d, metric, n, seed, idmap=False, **kw):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    ix, m = _pair(base, d, metric, x, rng, idmap=idmap, **kw)
    ids = (rng.permutation(10 * n)[:n].astype(np.int64) + 7) if idmap else None
    ix.add_with_ids(x, ids) if idmap else ix.add(x)
    m.add(x)
    assert ix.ntotal == n == ix.refine_base.ntotal == ix.refine_store.ntotal
    return ix, m, ids, rng


# ------------------------------------------------------------------------------------------------ model equality across dimensions
CASES = [
    (1, "SQ", L2, None), (1, "PQ", IP, 1), (5, "IVFSQ", IP, None),
    (16, "PQ", L2, 4), (16, "IVFPQ", IP, 2), (16, "SQ", IP, None), (16, "IVFSQ", L2, None),
    (17, "SQ", L2, None), (17, "IVFPQ", IP, 17), (100, "IVFPQ", L2, 4), (100, "SQ", IP, None),
    (128, "PQ", IP, 8), (128, "IVFPQ", L2, 16), (128, "SQ", L2, None), (128, "IVFSQ", IP, None),
    (129, "IVFSQ", L2, None), (129, "PQ", IP, 3), (768, "PQ", L2, 8), (768, "IVFSQ", IP, None),
    (2048, "SQ", L2, None), (2048, "IVFPQ", IP, 16),
]  # fmt: skip


@pytest.mark.parametrize("d,base,metric,M", CASES, ids=[f"d{c[0]}-{c[1]}-{'L2' if c[2] == L2 else 'IP'}" for c in CASES])
def test_results_equal_the_model(d, base, metric, M):
    n = 700 if d <= 129 else (300 if d == 768 else 200)
    idmap = d in (17, 128)
    ix, m, ids, rng = _filled(base, d, metric, n, 1000 + d + len(base), idmap=idmap, M=M)
    xq = rng.standard_normal((70, d)).astype(np.float32)
    exact = sqr.chains(metric, m.rows, xq)
    assert ix.k_factor == 1.0
    both = np.zeros(2, dtype=bool)
    for kf in (1, 4, 2.5):
        ix.k_factor = kf
        assert ix.k_factor == kf
        cand = m.base_search(xq, rfr.candidates(10, kf), nprobe=2)
        Dr, Ir = rfr.refine(metric, m.rows, xq, cand, 10, labels=ids, exact=exact)
        for nq in (7, 70):
            _same(*ix.search(xq[:nq], 10, nprobe=2), Dr[:nq], Ir[:nq], f"{base} d={d} k_factor={kf} nq={nq}")
        rows = rfr.refine(metric, m.rows, xq, cand, 10, exact=exact)[1]
        both |= [(((rows[rows >= 0] >> 4) & 1) == b).any() for b in (0, 1)]
        assert ix.get_stat("refine_candidates") == rfr.candidates(10, kf) and ix.get_stat("refine_query_chunk") == 70
        ki = ix.last_kernel_info()  # the stage's roofline: every candidate row once, whole
        assert ki["name"] == "refine_flat_kernel" and ki["grid"] == 70 and ki["bytes"] == 70.0 * min(rfr.candidates(10, kf), n) * 4 * _dp(d)
    assert both.all(), "the results hold rows with bit 4 of the row number clear and set"
    assert ix.get_stat("refine_store_bytes") >= n * _dp(d) * 4 and ix.get_stat("refine_store_bytes") % (_dp(d) * 4) == 0


def _dp(d):
    """FlatGeom's row pitch in floats: a power of two >= 8 up to 128, a multiple of 64 beyond"""
    if d <= 128:
        return max(8, 1 << (d - 1).bit_length())
    return (d + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------ kb at the limit
@pytest.mark.parametrize("base,metric", [("SQ", L2), ("IVFSQ", IP)])
def test_2048_candidates_and_the_limit(base, metric):
    mf = _mf()
    d, n = 16, 3000
    ix, m, _, rng = _filled(base, d, metric, n, 77, nlist=2)
    xq = rng.standard_normal((5, d)).astype(np.float32)
    ix.k_factor = 16
    D, I = ix.search(xq, 128, nprobe=2)
    assert ix.get_stat("refine_candidates") == 2048
    _same(D, I, *m.search(xq, 128, 16, nprobe=2), f"{base} kb = 2048")
    ix.k_factor = 16.01
    with pytest.raises(mf.FaissException, match=r"k = 128 with k_factor = 16.01 asks the base index for 2049 candidates: beyond the 2048"):
        ix.search(xq, 128, nprobe=2)
    for bad in (0.99, 0.0, -1.0, float("nan")):
        with pytest.raises(mf.FaissException, match="k_factor >= 1"):
            ix.k_factor = bad
    assert abs(ix.k_factor - 16.01) < 1e-5
    with pytest.raises(mf.FaissException, match="k > 0"):
        ix.search(xq, 0)
    _same(*ix.search(xq, 127, nprobe=2), *m.search(xq, 127, 16.01, nprobe=2), f"{base} kb = 2033")  # (127 * 16.01f = 2033.27)


# ------------------------------------------------------------------------------------------------ fewer candidates than kb
def test_short_lists_and_small_indexes_pad_the_tail():
    d = 12
    for metric in (L2, IP):
        ix, m, ids, rng = _filled("IVFSQ", d, metric, 300, 5 + metric, idmap=True, nlist=8)
        xq = rng.standard_normal((9, d)).astype(np.float32)
        ix.k_factor = 8
        assert max(ids_l.size for ids_l, _ in m.built()) < 250  # k = 250, kb = 2000: the one probed list runs out before either
        Dr, Ir = m.search(xq, 250, 8, nprobe=1, id_map=ids)
        assert (Ir[:, -1] == -1).all() and (Ir[:, 0] >= 0).all()
        D, I = ix.search(xq, 250, nprobe=1)
        _same(D, I, Dr, Ir, "nprobe = 1, lists shorter than kb")
        assert (D[I == -1] == (rfr.FLT_MAX if metric == L2 else -rfr.FLT_MAX)).all()
        # n < k
        ix, m, _, rng = _filled("PQ", d, metric, 5, 9 + metric, M=3)
        for kf in (1, 3):
            ix.k_factor = kf
            D, I = ix.search(xq, 10)
            _same(D, I, *m.search(xq, 10, kf), f"n = 5 < k = 10, k_factor {kf}")
            assert (I[:, :5] >= 0).all() and (I[:, 5:] == -1).all()
        # an empty, trained index
        ix, m = _pair("SQ", d, metric, xq, rng)
        D, I = ix.search(xq, 3)
        assert (I == -1).all() and (D == (rfr.FLT_MAX if metric == L2 else -rfr.FLT_MAX)).all()


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("idmap", [False, True])
def test_equal_exact_values_come_out_by_ascending_row(metric, idmap):
    """integer-lattice rows and queries: exact distances are small integers and tie across candidates; the IVF base's own order is
    (distance, probe rank, position), so rows arrive at the refine stage out of row order"""
    rng = np.random.default_rng(31 + metric)
    d, n, nlist = 8, 600, 4
    x = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
    ix, m = _pair("IVFSQ", d, metric, x, rng, nlist=nlist, idmap=idmap)
    ids = (rng.permutation(5000)[:n].astype(np.int64)) if idmap else None
    ix.add_with_ids(x, ids) if idmap else ix.add(x)
    m.add(x)
    xq = rng.integers(-2, 3, size=(20, d)).astype(np.float32)
    ix.k_factor = 6
    D, I = ix.search(xq, 40, nprobe=nlist)
    _same(D, I, *m.search(xq, 40, 6, nprobe=nlist, id_map=ids), "lattice")
    # ... and without the model: values in order, equal values by ascending ROW
    row_of = {int(v): r for r, v in enumerate(ids)} if idmap else None
    ties = 0
    for q in range(len(xq)):
        rows = np.array([row_of[int(v)] for v in I[q]]) if idmap else I[q]
        key = D[q] if metric == L2 else -D[q]
        assert (np.diff(key) >= 0).all()
        eq = np.diff(key) == 0
        ties += int(eq.sum())
        assert (np.diff(rows)[eq] > 0).all(), f"query {q}: equal values out of row order"
        base_rows = m.base_search(xq[q : q + 1], 240, nprobe=nlist)[0]
        assert set(rows.tolist()) <= set(base_rows.tolist())
    assert ties > 50, "the lattice is meant to tie"


# ------------------------------------------------------------------------------------------------ independent of the model
@pytest.mark.parametrize("base,metric,M", [("IVFPQ", L2, 4), ("SQ", IP, None), ("PQ", L2, 8), ("IVFSQ", IP, None)])
def test_with_every_row_a_candidate_the_result_is_the_oracles_flat_search(base, metric, M):
    d, n = 24, 200
    ix, m, _, rng = _filled(base, d, metric, n, 400 + metric, nlist=5, M=M)
    xq = rng.standard_normal((30, d)).astype(np.float32)
    Do, Io = orc.flat_search_naive(metric, m.rows, xq, 20, orc.PATH_PAIR)
    full, _ = orc.flat_search_naive(metric, m.rows, xq, n, orc.PATH_PAIR)
    assert (np.diff(full, axis=1) != 0).all(), "the seed must be tie-free"
    ix.k_factor = 10  # kb = 200 >= n
    _same(*ix.search(xq, 20, nprobe=5), Do, Io, f"{base}: kb >= n, nprobe = nlist")


def test_recall_with_refinement_is_not_below_the_bare_base():
    mf = _mf()
    rng = np.random.default_rng(2026)  # (a seed whose 2 x 50 x 1000 exact values hold no tie: checked below)
    d, n, nlist, M = 32, 1000, 8, 4
    centers = rng.standard_normal((20, d)).astype(np.float32) * 3
    x = (centers[rng.integers(0, 20, n)] + rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)
    xq = (centers[rng.integers(0, 20, 50)] + rng.standard_normal((50, d)).astype(np.float32)).astype(np.float32)
    for metric in (L2, IP):
        ix, m = _pair("IVFPQ", d, metric, x, rng, nlist=nlist, M=M)
        bare = mf.index_factory(d, f"IVF{nlist},PQ{M}", metric)
        bare.ivf_set_centroids(m.cent)
        bare.pq_set_centroids(m.cb)
        ix.add(x)
        bare.add(x)
        full, true = orc.flat_search_naive(metric, x, xq, n, orc.PATH_PAIR)
        assert (np.diff(full, axis=1) != 0).all(), "the seed must be tie-free: with ties the inequality below is not guaranteed"
        true = true[:, :10]
        ix.k_factor = 8
        _, Ir = ix.search(xq, 10, nprobe=4)
        _, Ib = bare.search(xq, 10, nprobe=4)
        rec = lambda I: np.mean([len(set(I[q].tolist()) & set(true[q].tolist())) / 10.0 for q in range(len(xq))])  # noqa: E731
        # the base's 10 best are among its 80 best, and the refine stage keeps every true neighbour it is given
        assert rec(Ir) >= rec(Ib), (rec(Ir), rec(Ib))
        assert rec(Ir) > rec(Ib), "on this set the compressed base does miss neighbours that re-ranking finds"


# ------------------------------------------------------------------------------------------------ selectors
@pytest.mark.parametrize("base,M", [("IVFSQ", None), ("PQ", 4)])
@pytest.mark.parametrize("idmap", [False, True])
def test_selectors_are_honoured_in_the_base_scan(base, M, idmap):
    d, n = 16, 500
    for metric in (L2, IP):
        ix, m, ids, rng = _filled(base, d, metric, n, 60 + metric, idmap=idmap, M=M)
        ext = ids if idmap else np.arange(n, dtype=np.int64)  # what the selector tests: the external id under IDMap, else the row
        xq = rng.standard_normal((11, d)).astype(np.float32)
        ix.k_factor = 3
        for keep in (ext % 3 == 0, ext % 50 == 1):  # (the second leaves 10 rows: fewer than kb)
            Dr, Ir = m.search(xq, 8, 3, nprobe=3, id_map=ids, keep=keep)
            for sel in (("bitmap", bitmap_from_ids(ext, keep)), ("batch", ext[keep])):
                D, I = ix.search(xq, 8, nprobe=3, sel=sel)
                assert np.isin(I[I >= 0], ext[keep]).all(), f"{sel[0]}: a rejected id appears"
                _same(D, I, Dr, Ir, f"{base} idmap={idmap} {sel[0]}")
        D, I = ix.search(xq, 8, nprobe=3, sel=("batch", np.array([10**7], dtype=np.int64)))
        assert (I == -1).all()


# ------------------------------------------------------------------------------------------------ batches, failures of add
@pytest.mark.parametrize("base,M", [("IVFPQ", 4), ("SQ", None)])
def test_batched_adds_give_the_results_of_one_add(base, M):
    mf = _mf()
    d, n = 20, 2128
    rng = np.random.default_rng(8)
    x = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((13, d)).astype(np.float32)
    one, m = _pair(base, d, L2, x, rng, M=M)
    many = _like(m, M)
    one.add(x)
    m.add(x)
    at = 0
    for bs in (1, 63, 1000, 1, 63, 1000):
        many.add(x[at : at + bs])
        at += bs
        assert many.ntotal == at == many.refine_store.ntotal == many.refine_base.ntotal
        if at in (64, 1064):  # a search between the adds: the staged rows reach the device, the store grows afterwards
            many.search(xq[:2], 3)
    assert at == n
    for ix in (one, many):
        ix.k_factor = 5
    Dr, Ir = m.search(xq, 10, 5, nprobe=2)
    _same(*one.search(xq, 10, nprobe=2), Dr, Ir, "one add")
    _same(*many.search(xq, 10, nprobe=2), Dr, Ir, "batches of 1, 63 and 1000")
    one.set_label_offset(1000)
    _same(*one.search(xq, 10, nprobe=2), Dr, Ir + 1000, "label_offset")


def test_device_resident_adds_do_the_same():
    import torch

    mf = _mf()
    d, n = 20, 2128
    rng = np.random.default_rng(8)
    x = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((13, d)).astype(np.float32)
    dev, m = _pair("IVFPQ", d, L2, x, rng, M=4)
    m.add(x)
    xt = torch.from_numpy(x).cuda()
    dev.add_torch(xt[:1500])
    dev.add_torch(xt[1500:])
    torch.cuda.synchronize()
    assert dev.ntotal == n == dev.refine_base.ntotal == dev.refine_store.ntotal
    dev.k_factor = 5
    _same(*dev.search(xq, 10, nprobe=2), *m.search(xq, 10, 5, nprobe=2), "add_torch")
    D, I = dev.search_torch(torch.from_numpy(xq).cuda(), 10, nprobe=2)
    _same(D.cpu().numpy(), I.cpu().numpy(), *m.search(xq, 10, 5, nprobe=2), "search_torch")
    with pytest.raises(mf.FaissException, match="add_with_ids not implemented for this type of index"):
        dev.add_torch(xt[:4], ids=torch.arange(4, dtype=torch.int64).cuda())
    assert dev.ntotal == n


def test_add_before_train_and_add_with_ids_fail_cleanly():
    mf = _mf()
    x = np.random.default_rng(1).standard_normal((50, 8)).astype(np.float32)
    for desc in ("IVF4,PQ2,RFlat", "SQ8,RFlat", "IDMap,IVF4,SQ8,RFlat", "PQ4,Refine(Flat)"):
        ix = mf.index_factory(8, desc, L2)
        assert not ix.is_trained and ix.ntotal == 0
        with pytest.raises(mf.FaissException, match="is_trained"):
            ix.add_with_ids(x, np.arange(50)) if desc.startswith("IDMap") else ix.add(x)
        assert ix.ntotal == 0 and ix.refine_base.ntotal == 0 and ix.refine_store.ntotal == 0
        with pytest.raises(mf.FaissException, match="is_trained"):
            ix.search(x[:2], 3)
    ix, m, _, _ = _filled("SQ", 8, L2, 50, 3)
    with pytest.raises(mf.FaissException, match="add_with_ids not implemented for this type of index"):
        ix.add_with_ids(x, np.arange(50))
    assert ix.ntotal == 50 and ix.refine_base.ntotal == 50 and ix.refine_store.ntotal == 50
    # train() trains the base; is_trained is the base's
    ix = mf.index_factory(8, "SQ8,RFlat", IP)
    ix.train(x)
    assert ix.is_trained and ix.refine_base.is_trained and ix.kind == mf.KIND_REFINE == 10
    vmin, vdiff = ix.refine_base.sq_trained()
    rmin, rdiff = sqr.train_range(x)
    assert (vmin == rmin).all() and (vdiff == rdiff).all()
    with pytest.raises(mf.FaissException, match="unknown option"):
        ix.set_option("no_such_option", 1)  # (options go to the base, which knows none of this name)


# ------------------------------------------------------------------------------------------------ placement
@pytest.mark.parametrize("base,M,idmap", [("PQ", 4, False), ("IVFSQ", None, True), ("IVFPQ", 2, False), ("SQ", None, True)])
def test_images_clones_and_refused_sharding(base, M, idmap, tmp_path):
    mf = _mf()
    d, n = 8, 120
    ix, m, ids, rng = _filled(base, d, IP if idmap else L2, n, 90, idmap=idmap, M=M)
    xq = rng.standard_normal((6, d)).astype(np.float32)
    ix.k_factor = 2.5
    want = m.search(xq, 7, 2.5, nprobe=2, id_map=ids)
    _same(*ix.search(xq, 7, nprobe=2), *want, "before")
    # the file the library writes is byte-equal to the Python writer's
    p1, p2 = str(tmp_path / "lib.index"), str(tmp_path / "py.index")
    mf.write_index(ix, p1)
    ref = m.image(k_factor=2.5, id_map=ids, path=p2)
    assert open(p1, "rb").read() == ref
    img = rfr.parse_refine(p1)
    assert img["base_kind"] == base and img["k_factor"] == 2.5 and np.array_equal(img["rows"].view(np.uint32), m.rows.view(np.uint32))
    # read_index of the Python writer's file searches equal
    back = mf.read_index(p2)
    assert back.kind == (mf.KIND_IDMAP if idmap else mf.KIND_REFINE) and back.ntotal == n and back.k_factor == 2.5 and back.is_trained
    assert back.refine_base.kind == ix.refine_base.kind and back.refine_store.ntotal == n
    _same(*back.search(xq, 7, nprobe=2), *want, "read_index")
    # ... and goes on taking rows
    extra = rng.standard_normal((9, d)).astype(np.float32)
    back.add_with_ids(extra, np.arange(9) + 10**6) if idmap else back.add(extra)
    m2 = rfr.Model(base, m.metric, d, cent=m.cent, cb=m.cb, vmin=m.vmin, vdiff=m.vdiff)
    m2.add(np.concatenate([m.rows, extra]))
    ids2 = np.concatenate([ids, np.arange(9) + 10**6]) if idmap else None
    _same(*back.search(xq, 7, nprobe=2), *m2.search(xq, 7, 2.5, nprobe=2, id_map=ids2), "read_index, then add")
    # clone_to_gpu(0): an independent copy; to_gpu(0) in place
    clone = ix.clone_to_gpu(0)
    assert clone.ntotal == n and clone.k_factor == 2.5
    _same(*clone.search(xq, 7, nprobe=2), *want, "clone_to_gpu(0)")
    ix.to_gpu(0)
    _same(*ix.search(xq, 7, nprobe=2), *want, "to_gpu(0)")
    # sharding is refused and leaves the index as it was
    for refused in (lambda: clone.shard_to_gpus([0, 0]), lambda: clone.clone_to_gpu(-1)):
        with pytest.raises(mf.FaissException, match="This index type is not implemented"):
            refused()
    assert clone.shard_info() is None and clone.ntotal == n
    _same(*clone.search(xq, 7, nprobe=2), *want, "after the refused sharding")


def test_sharded_factory_is_refused():
    """env MVS_DEVICES at creation: a fresh process, as the variable is read when the index is made"""
    code = (
        "import sys; sys.path.insert(0, %r); import mi355_faiss as mf\n"
        "for s in ('IDMap,IVF4,SQ8,RFlat', 'PQ4,Refine(Flat)'):\n"
        "    try:\n        mf.index_factory(8, s, 1)\n    except mf.FaissException as e:\n        print('REFUSED', e)\n"
    ) % os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, MVS_DEVICES="0,0"))
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("REFUSED") == 2 and out.stdout.count("This index type is not implemented") == 2


def test_malformed_images_are_refused(tmp_path):
    mf = _mf()
    rng = np.random.default_rng(17)
    d, n, nlist = 6, 40, 3
    x = rng.standard_normal((n, d)).astype(np.float32)
    cent = x[:nlist].copy()
    of_row, _ = sqr.assign(L2, cent, x)
    vmin, vdiff = sqr.train_range(sqr.residuals(cent, x, of_row))
    m = rfr.Model("IVFSQ", L2, d, cent=cent, vmin=vmin, vdiff=vdiff)
    m.add(x)
    path = str(tmp_path / "bad.index")
    m.image(path=path)
    assert mf.read_index(path).ntotal == n  # (the well-formed image is accepted)
    # base and store disagree in ntotal / d / metric
    for store, msg in ((rfr.flat_image(d, L2, x[:-1]), "disagree"), (rfr.flat_image(d, IP, x), "disagree"),
                       (rfr.flat_image(d + 1, L2, np.zeros((n, d + 1))), "disagree")):
        m.image(path=path, store_image=store)
        with pytest.raises(mf.FaissException, match=msg):
            mf.read_index(path)
    # an IVF base with a stored id outside [0, ntotal)
    for bad_id in (n, -1):
        lists = [(ids_l.copy(), codes_l) for ids_l, codes_l in m.built()]
        first = next(l for l, (ids_l, _) in enumerate(lists) if ids_l.size)
        lists[first][0][0] = bad_id
        rfr.write_refine(path, d, L2, sqr.write_ivfsq(None, d, L2, cent, vmin, vdiff, lists), x, 1.0)
        with pytest.raises(mf.FaissException, match=r"stored id %d outside \[0, %d\)" % (bad_id, n)):
            mf.read_index(path)
    # the second index is not a Flat image
    m.image(path=path, store_image=sqr.write_sq(None, d, L2, vmin, vdiff, sqr.encode(vmin, vdiff, x)))
    with pytest.raises(mf.FaissException, match="refine index is not a Flat image"):
        mf.read_index(path)
    # a base that is no scanning kind
    rfr.write_refine(path, d, L2, rfr.flat_image(d, L2, x), x, 1.0)
    with pytest.raises(mf.FaissException, match="IndexRefine over a base index of kind 1"):
        mf.read_index(path)


# ------------------------------------------------------------------------------------------------ factory strings
def test_factory_strings_and_refusals():
    mf = _mf()
    rng = np.random.default_rng(23)
    d, n = 8, 90
    x = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((4, d)).astype(np.float32)
    ids = np.arange(n, dtype=np.int64) * 5 + 3
    got = []
    for suffix, prefix in ((",RFlat", "IDMap,"), (",Refine(Flat)", "IDMap,"), (",RFlat", "IDMap2,"), (",Refine(Flat)", "IDMap2,")):
        ix, m = _pair("IVFPQ", d, L2, x, np.random.default_rng(5), M=2, idmap=True, suffix=suffix, prefix=prefix)
        assert ix.kind == mf.KIND_IDMAP and ix.index.kind == mf.KIND_REFINE and ix.refine_base.kind == mf.KIND_IVFPQ
        assert ix.index.refine_base.kind == mf.KIND_IVFPQ and ix.index.index is None and ix.refine_base.refine_base is None
        ix.add_with_ids(x, ids)
        ix.k_factor = 4
        got.append(ix.search(xq, 5, nprobe=2))
    m.add(x)
    for D, I in got:
        _same(D, I, *m.search(xq, 5, 4, nprobe=2, id_map=ids), "factory string variants")
    for desc in ("PQ4x8,RFlat", "IVF3,PQ2x8,Refine(Flat)", "SQ8,RFlat", "IVF3,SQ8,RFlat"):
        assert mf.index_factory(d, desc, IP).kind == mf.KIND_REFINE
    assert mf.index_factory(d, "Flat", L2).refine_base is None
    for desc in ("Flat,RFlat", "IVF4,Flat,RFlat", "HNSW16,RFlat", "HNSW16,SQ8,RFlat", "HNSW16_SQ8,Refine(Flat)", "IDMap,Flat,RFlat", "PQ4x4,RFlat",
                 "SQ4,RFlat", "IVF4_HNSW8,SQ8,RFlat", "OPQ4,PQ4,RFlat", "SQ8,Refine(SQ8)", "PQ4,Refine(PQ4)", "SQ8,RFlat,RFlat", "SQ8,Refine(Flat),RFlat",
                 "SQ8,RFlat,Refine(Flat)", "RFlat,SQ8,RFlat", "PQ200,RFlat"):
        with pytest.raises(mf.FaissException, match=NOT_YET):
            mf.index_factory(d if desc != "PQ200,RFlat" else 400, desc, L2)
    with pytest.raises(mf.FaissException, match=NOT_YET):
        mf.index_factory(d, "SQ8,RFlat", 2)  # METRIC_L1
    with pytest.raises(mf.FaissException, match="multiple of the number of subquantizers"):
        mf.index_factory(d, "PQ3,RFlat", L2)  # (the base's own message)
    for desc in ("RFlat", "Refine(Flat)"):
        with pytest.raises(mf.FaissException):
            mf.index_factory(d, desc, L2)


# ------------------------------------------------------------------------------------------------ the glue's path
def test_idmap_ivfsq_rflat_through_the_cpp_glue_path():
    """boundary_driver ingest: chunked AddFunction from two threads (buffered: the index needs training), AddFinaliseFunction (train + add),
    then the wrapper graph the glue sees -- an IndexRefine that is no IndexIVF -- and a search that honours the wrapper's k_factor member"""
    out = subprocess.run([DRIVER, "ingest", "3000", "8", "2", "IDMap,IVF8,SQ8,RFlat"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refine\tOK IndexRefine=1 IndexIVF=0 k_factor=64: 512/512 self-queries at distance 0" in out.stdout
    assert "ingest\tOK ntotal=3000" in out.stdout
