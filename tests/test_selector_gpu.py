"""Selector programs on the device (include/mi355_faiss.h "selector programs"; csrc/selector_lower.hip): IDSelectorRange / Array / All / Not /
And / Or / XOr as nested tuples through mi355_faiss.make_params.  The yardstick everywhere is the contract's promise: the same call on the same
index with ("batch", the admitted ids among the ids in the index) -- labels equal, distances equal as bit patterns; Flat L2 / inner product
also against the CPU oracle with that batch.  The admitted ids come from the numpy model of tests/selector_reference.py."""

import gc
import os
import subprocess

import numpy as np
import pytest

import pq_reference as pqr
import selector_reference as selr
import sq_reference as sqr
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
L2, IP, L1 = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 3000, 16


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss

    return mi355_faiss


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(7)
    xb = rng.standard_normal((N, D)).astype(np.float32)
    xq = rng.standard_normal((33, D)).astype(np.float32)
    ext = (rng.permutation(4 * N)[:N] + 5).astype(np.int64)  # external ids under IDMap
    return xb, xq, ext


def _same(got, want, what):
    (Dg, Ig), (Dw, Iw) = got, want
    assert np.array_equal(Ig, Iw), f"{what}: labels differ in {(Ig != Iw).sum()} slots"
    assert np.array_equal(Dg.view(np.uint32), Dw.view(np.uint32)), f"{what}: distances differ in {(Dg != Dw).sum()} slots"


def _trees(rng, ids, k):
    """the trees of the issue over the ids of an index: each leaf alone, its negation, and / or / xor of range x batch, and(range, not(array)),
    a depth-5 random tree, all, not(all), one admitting exactly one id and one admitting exactly k - 1"""
    lo, hi = np.sort(rng.choice(ids, 2, replace=False))
    some = rng.permutation(ids)[: ids.size // 3]
    few = rng.permutation(ids)[:40]
    nonneg = ids[ids >= 0]
    bits = selr.bitmap_of(nonneg[rng.random(nonneg.size) < 0.4])
    leaves = [("range", int(lo), int(hi)), ("batch", some), ("array", few), ("bitmap", bits), ("all",)]
    trees = [(t[0], t) for t in leaves] + [("not " + t[0], ("not", t)) for t in leaves]
    rg, bt = leaves[0], leaves[1]
    trees += [(op + "(range, batch)", (op, rg, bt)) for op in ("and", "or", "xor")]
    trees.append(("and(range, not(array))", ("and", rg, ("not", ("array", few)))))
    trees.append(("random depth 5", selr.random_tree(rng, np.concatenate([ids, [-3, 0, 1 << 40]]), 5)))
    one = int(ids[ids.size // 2])
    trees.append(("exactly one", ("and", ("range", one, one + 1), ("not", ("batch", np.array([one + 1]))))))
    if k > 1:
        pick = np.unique(rng.permutation(ids)[: k - 1])
        trees.append(("exactly k - 1", ("xor", ("array", np.concatenate([pick, few])), ("batch", np.setdiff1d(few, pick)))))
    return trees


def _cent(xb, nlist=8):
    return xb[:: len(xb) // nlist][:nlist].copy()


def _build(mf, desc, metric, xb, ext, rng):
    """the index with its parameters set (coded kinds through the accessors, as their own tests do) and the ids its selectors test"""
    d = xb.shape[1]
    ix = mf.index_factory(d, desc, metric)
    mapped = desc.startswith("IDMap")
    core = ix.refine_base if "RFlat" in desc else ix
    if "PCA" in desc:
        ix.train(xb)
    elif "_HNSW" in desc or desc.endswith("HNSW16,SQ8"):
        ix.train(xb)
    else:
        if "IVF" in desc:
            core.ivf_set_centroids(_cent(xb))
        if "PQ4" in desc:
            core.pq_set_centroids(pqr.synthetic_codebooks(rng, 4, d // 4))
        if "SQ8" in desc:
            res = xb - _cent(xb)[sqr.assign(metric, _cent(xb), xb)[0]] if "IVF" in desc else xb
            core.sq_set_trained(*sqr.train_range(res))
    ix.add_with_ids(xb, ext) if mapped else ix.add(xb)
    return ix, (ext if mapped else np.arange(len(xb), dtype=np.int64))


KINDS = [("Flat", L2), ("Flat", IP), ("IDMap,Flat", L2), ("Flat", L1), ("IVF8,Flat", L2), ("IDMap,IVF8,Flat", L2), ("IVF8_HNSW8,Flat", L2),
         ("HNSW16", L2), ("PQ4", L2), ("IVF8,PQ4", L2), ("SQ8", L2), ("IVF8,SQ8", L2), ("HNSW16,SQ8", L2), ("SQ8,RFlat", L2), ("PCA8,Flat", L2)]


@pytest.mark.parametrize("desc,metric", KINDS)
def test_every_tree_equals_the_batch_of_its_admitted_ids(mf, data, desc, metric):
    xb, xq, ext = data
    rng = np.random.default_rng(sum(map(ord, desc)) + metric)
    ix, ids = _build(mf, desc, metric, xb, ext, rng)
    kw = dict(nprobe=4) if "IVF" in desc else dict(efSearch=64) if "HNSW16" in desc else {}
    oracle_ix = None
    if desc in ("Flat", "IDMap,Flat") and metric in (L2, IP):
        oracle_ix = orc.Index(D, desc, metric)
        oracle_ix.add_with_ids(xb, ext) if desc.startswith("IDMap") else oracle_ix.add(xb)
    for nq, k in ((1, 1), (33, 10), (33, 1), (1, 10)):
        for name, tree in _trees(rng, ids, k):
            adm = selr.admitted(ids, tree)
            what = f"{desc} metric {metric} nq {nq} k {k} {name} ({adm.size} admitted)"
            got = ix.search(xq[:nq], k, sel=tree, **kw)
            assert ix.get_stat("sel_admitted") == adm.size or len(selr.postfix(tree)) == 1, what
            want = ix.search(xq[:nq], k, sel=("batch", adm), **kw)
            _same(got, want, what)
            if adm.size == 0:  # not(all): every label -1, every distance the kind's neutral fill
                assert (got[1] == -1).all() and np.unique(got[0].view(np.uint32)).size == 1, what
            if adm.size < k and "HNSW16" not in desc and "IVF" not in desc:
                assert ((got[1] >= 0).sum(axis=1) == adm.size).all(), what
            if oracle_ix is not None and (nq, k) == (33, 10):
                _same(got, oracle_ix.search(xq[:nq], k, sel=("batch", adm)), what + " vs the oracle")


def test_flat_selector_program_on_the_coarse_filter_row_mask(mf):
    """the shape of tests/test_collect_gpu.py's selector case (n = 150 000, d = 128, nq = 300, k = 10): the lowered selector becomes the bf16
    coarse filter's one-bit-per-row mask"""
    rs = np.random.RandomState(47)
    n, d, nq, k = 150_000, 128, 300, 10
    xb = rs.rand(n, d).astype(np.float32)
    xq = rs.rand(nq, d).astype(np.float32)
    ix = mf.index_factory(d, "Flat", L2)
    ix.set_option("prefilter", 2)
    for i0 in range(0, n, 1 << 16):
        ix.add(xb[i0 : i0 + (1 << 16)])
    ids = np.arange(n, dtype=np.int64)
    tree = ("and", ("range", 16, n), ("not", ("batch", ids[rs.rand(n) < 0.7])))  # (about 0.3 n admitted, spread over the rows as in that test)
    adm = selr.admitted(ids, tree)
    got = ix.search(xq, k, sel=tree)
    assert ix.last_kernel_info()["name"] == "flat_bf16_collect_kernel" and ix.get_stat("sel_lowered") == 1 and ix.get_stat("sel_admitted") == adm.size
    _same(got, ix.search(xq, k, sel=("batch", adm)), "coarse filter")
    _same((got[0][:64], got[1][:64]), orc.flat_search(L2, xb, xq[:64], k, sel=("batch", adm)), "coarse filter vs the oracle")


@pytest.mark.parametrize("desc", ["Flat", "IDMap,Flat", "IVF8,Flat", "PQ4"])
def test_both_lowerings_give_the_same_results(mf, data, desc):
    xb, xq, ext = data
    rng = np.random.default_rng(3)
    ix, ids = _build(mf, desc, L2, xb, ext, rng)
    kw = dict(nprobe=4) if "IVF" in desc else {}
    tree = ("and", ("range", int(np.median(ids)), int(ids.max()) + 1), ("not", ("batch", rng.permutation(ids)[:100])))
    adm = selr.admitted(ids, tree)
    want = ix.search(xq, 10, sel=("batch", adm), **kw)
    assert ix.get_stat("sel_lowered") == 0
    ix.set_option("sel_bitmap_cap_bytes", 1)
    as_batch = ix.search(xq, 10, sel=tree, **kw)
    assert ix.get_stat("sel_lowered") == 2 and ix.get_stat("sel_admitted") == adm.size
    ix.set_option("sel_bitmap_cap_bytes", 1 << 30)
    as_bitmap = ix.search(xq, 10, sel=tree, **kw)
    assert ix.get_stat("sel_lowered") == 1 and ix.get_stat("sel_admitted") == adm.size
    _same(as_batch, want, desc + " lowered to a batch")
    _same(as_bitmap, want, desc + " lowered to a bitmap")
    ix.set_option("sel_bitmap_cap_bytes", 0)
    _same(ix.search(xq, 10, sel=tree, **kw), want, desc + " automatic cap")
    assert ix.get_stat("sel_lowered") == 1  # (ids below 4 n: well inside the automatic cap's 1 MiB floor)
    # a one-leaf program of a plain selector takes the plain path: no evaluation
    _same(ix.search(xq, 10, sel=("program", [(mf.SELOP_ARRAY, adm, 0, 0)]), **kw), want, desc + " one ARRAY leaf")
    assert ix.get_stat("sel_lowered") == 0


def test_idmap_ids_negative_huge_and_duplicate(mf, data):
    xb, xq, _ = data
    rng = np.random.default_rng(5)
    ids = np.concatenate([-rng.permutation(1000) - 1, (1 << 40) + rng.permutation(1000), rng.permutation(900), rng.permutation(100)[:100]]).astype(np.int64)
    ids[-100:] = ids[2000:2100]  # duplicate external ids
    ix = mf.index_factory(D, "IDMap,Flat", L2)
    ix.add_with_ids(xb, ids)
    cases = [("negatives", ("range", -500, 0), 2), ("2^40 + i", ("range", (1 << 40) + 10, (1 << 40) + 700), 2), ("small", ("range", 0, 500), 1),
             ("mixed", ("not", ("range", -900, (1 << 40) + 100)), 2), ("duplicates", ("and", ("array", ids[2000:2050]), ("all",)), 1)]
    for name, tree, lowered in cases:
        adm = selr.admitted(ids, tree)
        got = ix.search(xq, 10, sel=tree)
        assert ix.get_stat("sel_lowered") == lowered and ix.get_stat("sel_admitted") == adm.size, name
        _same(got, ix.search(xq, 10, sel=("batch", adm)), name)
    assert selr.admitted(ids, cases[-1][1]).size == 100  # (each of the 50 ids is carried by two rows)


def test_staged_rows_and_the_empty_index(mf, data):
    xb, xq, ext = data
    for desc in ("Flat", "IDMap,Flat"):
        ix = mf.index_factory(D, desc, L2)
        tree = ("not", ("range", 10, 1 << 50))
        D0, I0 = ix.search(xq, 3, sel=tree)  # empty: nothing is launched; where the kind asks for a selector at all, the empty batch
        assert (I0 == -1).all() and ix.get_stat("sel_lowered") in (0, 2) and ix.get_stat("sel_admitted") == 0
        ids = ext if desc.startswith("IDMap") else np.arange(N, dtype=np.int64)
        ix.add_with_ids(xb[:2000], ids[:2000]) if desc.startswith("IDMap") else ix.add(xb[:2000])
        ix.search(xq[:1], 1)
        ix.add_with_ids(xb[2000:], ids[2000:]) if desc.startswith("IDMap") else ix.add(xb[2000:])  # staged: no flush before the search
        tree = ("range", int(np.sort(ids)[2500]), int(ids.max()) + 1)
        adm = selr.admitted(ids, tree)
        assert np.isin(adm, ids[2000:]).any()
        got = ix.search(xq, 10, sel=tree)
        assert ix.get_stat("sel_admitted") == adm.size
        _same(got, ix.search(xq, 10, sel=("batch", adm)), desc + " staged rows")


@pytest.mark.parametrize("n", [63, 64, 65])
@pytest.mark.parametrize("cap", [1, 0])
def test_ballot_tail(mf, data, n, cap):
    xb, xq, _ = data
    ids = np.arange(n, dtype=np.int64) * 3 - 30
    ix = mf.index_factory(D, "IDMap,Flat", L2)
    ix.add_with_ids(xb[:n], ids)
    ix.set_option("sel_bitmap_cap_bytes", cap)
    for tree in (("all",), ("range", int(ids[n - 1]), int(ids[n - 1]) + 1), ("not", ("batch", ids[: n - 1])), ("range", int(ids[n - 2]), 1 << 40)):
        adm = selr.admitted(ids, tree)
        got = ix.search(xq, 5, sel=tree)
        assert ix.get_stat("sel_admitted") == adm.size
        _same(got, ix.search(xq, 5, sel=("batch", adm)), f"n = {n} cap = {cap} {tree[0]}")


@pytest.mark.parametrize("desc", ["BFlat", "IDMap,BFlat"])
def test_binary_search_and_range_search(mf, data, desc):
    rng = np.random.default_rng(11)
    bb = rng.integers(0, 256, (N, 8), dtype=np.uint8)
    bq = rng.integers(0, 256, (33, 8), dtype=np.uint8)
    ext = data[2]
    ix = mf.index_binary_factory(64, desc)
    ids = ext if desc.startswith("IDMap") else np.arange(N, dtype=np.int64)
    ix.add_with_ids(bb, ids) if desc.startswith("IDMap") else ix.add(bb)
    for cap in (0, 1):
        ix.set_option("sel_bitmap_cap_bytes", cap)
        for name, tree in _trees(rng, ids, 10):
            adm = selr.admitted(ids, tree)
            Dg, Ig = ix.search(bq, 10, sel=tree)
            assert ix.get_stat("sel_admitted") == adm.size or len(selr.postfix(tree)) == 1, name
            Dw, Iw = ix.search(bq, 10, sel=("batch", adm))
            assert np.array_equal(Ig, Iw) and np.array_equal(Dg, Dw), f"{desc} {name}"
            got, want = ix.range_search(bq, 24, sel=tree), ix.range_search(bq, 24, sel=("batch", adm))
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), f"{desc} range_search {name}"


@pytest.mark.parametrize("desc", ["Flat", "IVF8,Flat"])
def test_range_search(mf, data, desc):
    xb, xq, ext = data
    rng = np.random.default_rng(13)
    ix, ids = _build(mf, desc, L2, xb, ext, rng)
    kw = dict(nprobe=4) if "IVF" in desc else {}
    tree = ("and", ("range", 500, 2500), ("not", ("batch", rng.permutation(ids)[:300])))
    adm = selr.admitted(ids, tree)
    radius = float(np.median(ix.search(xq, 50, **kw)[0][:, -1]))
    got, want = ix.range_search(xq, radius, sel=tree, **kw), ix.range_search(xq, radius, sel=("batch", adm), **kw)
    assert got[0][-1] > 0 and np.isin(got[2], adm).all()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("desc", ["Flat", "IDMap,PQ4", "IVF8,SQ8", "IDMap,IVF8,Flat"])
@pytest.mark.parametrize("negate", [False, True])
def test_remove_ids(mf, data, desc, negate, tmp_path):
    xb, xq, ext = data
    kw = dict(nprobe=4) if "IVF" in desc else {}
    twins = [_build(mf, desc, L2, xb, ext, np.random.default_rng(17)) for _ in range(2)]
    ids = twins[0][1]
    lo, hi = np.sort(ids)[[700, 2200]]
    tree = ("range", int(lo), int(hi))
    tree = ("not", tree) if negate else tree
    adm = selr.admitted(ids, tree)
    (a, _), (b, _) = twins
    na, nb = a.remove_ids(tree), b.remove_ids(("batch", adm))
    assert na == nb == adm.size and a.ntotal == b.ntotal == N - adm.size
    _same(a.search(xq, 10, **kw), b.search(xq, 10, **kw), desc + " after remove_ids")
    mf.write_index(a, str(tmp_path / "a.index"))
    mf.write_index(b, str(tmp_path / "b.index"))
    assert (tmp_path / "a.index").read_bytes() == (tmp_path / "b.index").read_bytes()
    assert a.remove_ids(("not", ("all",))) == 0 and a.ntotal == N - adm.size  # no member: nothing is touched


def test_sharded_flat(mf, data):
    xb, xq, _ = data
    one = mf.index_factory(D, "Flat", IP)
    one.add(xb)
    sh = mf.index_factory(D, "Flat", IP)
    sh.add(xb)
    sh.shard_to_gpus([0, 0])
    ids = np.arange(N, dtype=np.int64)
    rng = np.random.default_rng(19)
    for name, tree in _trees(rng, ids, 10):
        _same(sh.search(xq, 10, sel=tree), one.search(xq, 10, sel=("batch", selr.admitted(ids, tree))), "sharded " + name)


def test_malformed_programs_fail_and_leave_the_index_alone(mf, data):
    xb, xq, ext = data
    ix = mf.index_factory(D, "IDMap,Flat", L2)
    ix.add_with_ids(xb, ext)
    before = ix.search(xq, 10)
    A, R, NOT, AND = mf.SELOP_ALL, mf.SELOP_RANGE, mf.SELOP_NOT, mf.SELOP_AND
    ids = np.arange(4, dtype=np.int64)
    bad = [([(A, None, 0, 0), (42, None, 0, 0)], "node 1", "unknown op 42"), ([(NOT, None, 0, 0)], "node 0", "stack underflow"),
           ([(A, None, 0, 0), (AND, None, 0, 0)], "node 1", "stack underflow"), ([(A, None, 0, 0), (R, None, 0, 9)], "node 1", "2 values left"),
           ([], "node 0", "empty"), ([(A, None, 0, 0)] * 33 + [(AND, None, 0, 0)] * 32, "node 64", "more than 64 nodes"),
           ([(mf.SELOP_BATCH, ids, 0, 0, -2)], "node 0", "n < 0"), ([(mf.SELOP_ARRAY, None, 0, 0, 3)], "node 0", "NULL data with n > 0")]
    for nodes, where, why in bad:
        for call in (lambda s: ix.search(xq, 10, sel=s), lambda s: ix.range_search(xq, 1.0, sel=s), lambda s: ix.remove_ids(s)):
            with pytest.raises(mf.FaissException) as e:
                call(("program", nodes))
            assert "selector program" in str(e.value) and where in str(e.value) and why in str(e.value), (nodes, str(e.value))
    with pytest.raises(mf.FaissException):  # still an error, still unknown
        ix.remove_ids(None)
    p, _ = mf.make_params()
    p.sel_kind = 9
    import ctypes as C

    assert mf._L.mvs_index_search(ix._h, 1, xq.ctypes.data_as(C.c_void_p), 1, before[0].ctypes.data_as(C.c_void_p), before[1].ctypes.data_as(C.c_void_p),
                                  C.byref(p)) != 0 and "unknown selector kind 9" in mf._L.mvs_last_error().decode()
    assert ix.ntotal == N
    _same(ix.search(xq, 10), before, "after the errors")
    assert ix.remove_ids(("range", int(ext.min()), int(ext.min()) + 1)) == 1 and ix.ntotal == N - 1  # (and a well-formed program still works)


@pytest.mark.parametrize("desc", ["IDMap,Flat", "IVF8,Flat"])
def test_adaptor_classes_through_the_boundary_driver(desc):
    exe = os.path.join(ROOT, "duckdb-faiss-ext_amd", "host", "boundary_driver")
    assert os.path.exists(exe), "host/boundary_driver is built by build()"
    r = subprocess.run([exe, "selectors", "3000", "16", "9", desc], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and "SELECTORS OK" in r.stdout, r.stdout[-3000:]


def test_device_memory_returns(mf, data):
    xb, xq, ext = data
    gc.collect()
    keeper = mf.index_factory(8, "Flat", L2)
    start = keeper.get_stat("device_bytes_live")
    tree = ("and", ("range", 100, 1 << 41), ("not", ("batch", ext[:50])))
    for desc in ("Flat", "IDMap,Flat", "IVF8,Flat", "PQ4", "IVF8,SQ8", "HNSW16"):
        ix, ids = _build(mf, desc, L2, xb, ext, np.random.default_rng(23))
        for cap in (1, 0):
            ix.set_option("sel_bitmap_cap_bytes", cap)
            ix.search(xq, 5, sel=tree)
        assert keeper.get_stat("device_bytes_live") > start
        del ix
    bx = mf.index_binary_factory(64, "BFlat")
    bx.add(np.zeros((100, 8), dtype=np.uint8))
    bx.search(np.zeros((1, 8), dtype=np.uint8), 1, sel=("not", ("range", 0, 5)))
    del bx
    gc.collect()
    assert keeper.get_stat("device_bytes_live") == start
