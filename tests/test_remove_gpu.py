"""remove_ids on the device (include/mi355_faiss.h "remove_ids") against two oracles:
  (a) the image: loads(write_index(after)) equals tests/remove_reference.py applied to loads(write_index(before)), floats as bit patterns
      (the code kinds, which tests/faiss_format.py does not parse: their codes and lists through the accessors, against the same model);
  (b) a FRESH index built through the existing paths from the model's surviving rows in the model's order: search (k = 1, 10, 100;
      7 and 33 queries: the per-pair and the BLAS branch) and range_search, where served, give equal labels and bit-equal distances.
The shapes are the smallest that reach each hazard: both sides of every layout-parity change of the pair-interleaved Flat store (row 0, 16
and 32 leading rows), d on both sides of 128, a removed run longer than a workgroup's tile, empty / one-row / emptied inverted lists,
duplicated rows on an integer lattice so that list order decides ties."""
import functools
import os
import subprocess

import numpy as np
import pytest

import faiss_format as ff
import pq_reference as pqr
import remove_reference as rr

pytestmark = pytest.mark.gpu

L2, IP, L1 = 1, 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = "remove_ids not implemented for this type of index"


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss as m

    assert m.device_count() >= 1
    return m


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def image_of(mf, ix, tmp_path, name="a.index"):
    p = str(tmp_path / name)
    mf.write_index(ix, p)
    with open(p, "rb") as f:
        return ff.loads(f.read())


@functools.lru_cache(maxsize=None)
def rows_of(d, n, lattice=False):
    rng = np.random.default_rng(31 * d + n)
    if lattice:
        xb = rng.integers(-1, 2, size=(n, d)).astype(np.float32)
    else:
        xb = rng.random((n, d), dtype=np.float32) - np.float32(0.25)
    dup = np.arange(n // 2, n, 5)[: n // 10]  # about a tenth of the rows duplicated: ties
    xb[dup] = xb[: dup.size]
    xb.setflags(write=False)
    return xb


@functools.lru_cache(maxsize=None)
def queries_of(d, nq):
    rng = np.random.default_rng(977 * d + nq)
    xq = rng.random((nq, d), dtype=np.float32) - np.float32(0.25)
    xq.setflags(write=False)
    return xq


def selectors(gone, top):
    """both selector kinds for the ids in `gone`: a batch with duplicates and absent ids, a bitmap that ends at the last member (shorter
    than ntotal / 8 unless the last ids go)"""
    gone = np.asarray(gone, dtype=np.int64)
    batch = np.concatenate([gone, gone[:5], [top + 1000, -7]]).astype(np.int64)
    bits = np.zeros(int(gone.max()) // 8 + 1 if gone.size else 1, np.uint8)
    for v in gone.tolist():
        bits[v >> 3] |= 1 << (v & 7)
    return {"batch": ("batch", batch), "bitmap": ("bitmap", bits)}


def assert_same_answers(a, b, d, ranged, what, ks=(1, 10, 100), **kw):
    assert a.ntotal == b.ntotal, what
    if a.ntotal == 0:
        return
    for nq in (7, 33):
        xq = queries_of(d, nq)
        for k in ks:
            Da, Ia = a.search(xq, k, **kw)
            Db, Ib = b.search(xq, k, **kw)
            assert np.array_equal(Ia, Ib), f"{what}: labels differ at nq {nq} k {k}"
            assert np.array_equal(u32(Da), u32(Db)), f"{what}: distances are not bit-equal at nq {nq} k {k}"
        if ranged:
            Db, _ = b.search(xq, min(10, b.ntotal), **kw)
            radius = np.float32(np.median(Db[:, -1]))
            ga, gb = a.range_search(xq, radius, **kw), b.range_search(xq, radius, **kw)
            assert gb[0][-1] > 0, what
            assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[2], gb[2]) and np.array_equal(u32(ga[1]), u32(gb[1])), f"{what}: range_search differs at nq {nq}"


def assert_same_up_to_ties(a, b, d, what, **kw):
    """distances bit-equal; a label may differ only inside a run of bit-equal distances or at the k-th place.  IVF<n>,Flat orders equal
    distances by STORED id (FAISS's heap compares (value, id) pairs), and under IDMap a fresh index numbers its stored ids by arrival where
    remove_ids keeps the survivors' relative numbering"""
    for nq in (7, 33):
        xq = queries_of(d, nq)
        for k in (1, 10, 100):
            Da, Ia = a.search(xq, k, **kw)
            Db, Ib = b.search(xq, k, **kw)
            assert np.array_equal(u32(Da), u32(Db)), f"{what}: distances are not bit-equal at nq {nq} k {k}"
            tied = np.zeros(Ia.shape, dtype=bool)
            tied[:, -1] = True
            eq = u32(Da)[:, 1:] == u32(Da)[:, :-1]
            tied[:, 1:] |= eq
            tied[:, :-1] |= eq
            assert not ((Ia != Ib) & ~tied).any(), f"{what}: labels differ outside ties at nq {nq} k {k}"


# ---------------------------------------------------------------------------------------------------------------- Flat
def flat_pattern(name, n):
    odd = list(range(3, n, 3))
    if (n - len(odd)) % 2 == 0:  # an odd survivor count
        odd = odd[:-1]
    return {
        "row0": [0],
        "lead16": list(range(16)),
        "lead32": list(range(32)),
        "last": [n - 1],
        "every_other": list(range(0, n, 2)),
        "run": list(range(n // 4, n // 4 + 300)) if n > 700 else list(range(n // 4, n // 4 + 100)),  # longer than a workgroup's 256 lanes of one row word
        "all": list(range(n)),
        "none": [],
        "odd": odd,
    }[name]


ALL_PATTERNS = ["row0", "lead16", "lead32", "last", "every_other", "run", "all", "none", "odd"]
FLAT_CASES = [(L2, 64, 1000, p) for p in ALL_PATTERNS] + [(L2, 132, 1000, p) for p in ALL_PATTERNS]
FLAT_CASES += [(L2, d, n, p) for d, n in ((1, 1000), (5, 257), (128, 257), (768, 257)) for p in ("row0", "lead16", "every_other", "odd")]
FLAT_CASES += [(IP, 64, 1000, p) for p in ("row0", "lead16", "run")] + [(IP, 132, 257, "every_other"), (L1, 5, 257, "lead16")]


@pytest.mark.parametrize("metric,d,n,pattern", FLAT_CASES)
def test_flat(mf, tmp_path, metric, d, n, pattern):
    xb = rows_of(d, n)
    gone = flat_pattern(pattern, n)
    if pattern == "odd":
        assert (n - len(gone)) % 2 == 1
    for kind, sel in selectors(gone, n).items() if gone else [("batch", ("batch", np.array([n + 5, -1], np.int64)))]:
        ix = mf.index_factory(d, "Flat", metric)
        ix.add(xb)
        before = image_of(mf, ix, tmp_path)
        want, removed = rr.remove_image(before, sel)
        assert removed == len(gone)
        assert ix.remove_ids(sel) == removed, f"{pattern} {kind}"
        assert ix.ntotal == n - removed
        assert rr.same_image(image_of(mf, ix, tmp_path, "b.index"), want), f"{pattern} {kind}: the image differs from the model"
        fresh = mf.index_factory(d, "Flat", metric)
        rows, _, _ = rr.survivors(want)
        if len(rows):
            fresh.add(rows)
        assert_same_answers(ix, fresh, d, metric != L1, f"Flat d {d} {pattern} {kind}")
        if pattern == "all":  # still usable: add numbers from the new ntotal
            ix.add(xb[:40])
            fresh.add(xb[:40])
            assert_same_answers(ix, fresh, d, True, "Flat refilled after removing every row")


@pytest.mark.parametrize("desc", ["IDMap,Flat", "IDMap2,Flat"])
@pytest.mark.parametrize("d,n", [(64, 1000), (132, 257)])
def test_idmap_flat(mf, tmp_path, desc, d, n):
    xb = rows_of(d, n)
    ext = (np.arange(n, dtype=np.int64) * 3 + 11) % 701  # duplicates once n > 701: every row carrying a member id goes
    gone = np.unique(ext[::7])
    for kind, sel in selectors(gone, int(ext.max())).items():
        ix = mf.index_factory(d, desc, L2)
        ix.add_with_ids(xb, ext)
        want, removed = rr.remove_image(image_of(mf, ix, tmp_path), sel)
        assert removed == int(np.isin(ext, gone).sum()) and removed > gone.size * (n > 701)
        assert ix.remove_ids(sel) == removed
        assert ix.ntotal == n - removed and ix.index.ntotal == n - removed
        assert rr.same_image(image_of(mf, ix, tmp_path, "b.index"), want), f"{desc} {kind}"
        rows, _, labels = rr.survivors(want)
        fresh = mf.index_factory(d, desc, L2)
        fresh.add_with_ids(rows, labels)
        assert_same_answers(ix, fresh, d, True, f"{desc} d {d} {kind}")
        keep = ("batch", labels[::2])  # a search selector on the external ids still works
        for k in (1, 10):
            a, b = ix.search(queries_of(d, 7), k, sel=keep), fresh.search(queries_of(d, 7), k, sel=keep)
            assert np.array_equal(a[1], b[1]) and np.array_equal(u32(a[0]), u32(b[0]))


def test_flat_label_offset_names_the_rows(mf):
    d, n = 64, 300
    ix = mf.index_factory(d, "Flat", L2)
    ix.set_label_offset(1000)
    ix.add(rows_of(d, n))
    assert ix.remove_ids(("batch", [0, 5, 299])) == 0  # the ids are label_offset + row
    assert ix.remove_ids(("batch", [1000, 1005, 1299, 1300])) == 3 and ix.ntotal == n - 3
    fresh = mf.index_factory(d, "Flat", L2)
    fresh.set_label_offset(1000)
    fresh.add(np.delete(rows_of(d, n), [0, 5, 299], axis=0))
    assert_same_answers(ix, fresh, d, True, "label offset")


def test_flat_order_of_operations(mf, tmp_path):
    d, n = 64, 1000
    xb = rows_of(d, n)
    more = rows_of(d, 6000)
    ix = mf.index_factory(d, "Flat", L2)
    for i0 in range(0, n, 100):  # small adds: rows are still staged (lazy_adds) when remove_ids is called
        ix.add(xb[i0 : i0 + 100])
    keep1 = np.setdiff1d(np.arange(n), np.arange(0, n, 3))
    assert ix.remove_ids(("batch", np.arange(0, n, 3))) == n - keep1.size
    cur = xb[keep1]
    ix.add(more)  # beyond the store's capacity: grow
    cur = np.concatenate([cur, more])
    gone2 = np.arange(5, cur.shape[0], 11)
    assert ix.remove_ids(selectors(gone2, cur.shape[0])["bitmap"]) == gone2.size  # remove, add, remove
    cur = np.delete(cur, gone2, axis=0)
    fresh = mf.index_factory(d, "Flat", L2)
    fresh.add(cur)
    assert_same_answers(ix, fresh, d, True, "remove, add, remove")
    p = str(tmp_path / "c.index")
    mf.write_index(ix, p)
    assert_same_answers(mf.read_index(p), fresh, d, True, "remove, write_index, read_index")
    clone = ix.clone_to_gpu(0)
    assert_same_answers(clone, fresh, d, True, "a clone after removal")
    ix.to_gpu(0)
    assert_same_answers(ix, fresh, d, False, "to_gpu after removal", ks=(10,))
    clone.shard_to_gpus([0, 0])
    assert_same_answers(clone, fresh, d, False, "shard_to_gpus after removal", ks=(10,))


def test_flat_derived_stores_are_rebuilt(mf):
    """a search BEFORE the removal has built the bf16 / int8 coarse stores and the shadow clustering; the search AFTER must not read them"""
    from oracle import oracle as orc

    d, n, nq, k = 64, 300_000, 600, 10
    xb = orc.synth_clustered(n, d, 7, n_centers=256, sigma=0.05)
    xb = np.round(xb * 8) / 8
    xq = xb[np.random.RandomState(3).randint(0, n, nq)].copy()
    gone = np.concatenate([np.arange(16), np.arange(100, n, 10)])

    def make(rows):
        ix = mf.index_factory(d, "Flat", L2)
        ix.set_option("prefilter", 2)
        ix.add(rows)
        return ix

    ix = make(xb)
    ix.search(xq, k)  # the coarse filter: builds the bf16 / int8 stores
    assert ix.collect_stats()["queries"] > 0, ix.collect_stats()
    ix.set_option("flat_shadow", 1)
    for _ in range(2):
        ix.search(xq, k)  # builds the shadow clustering and answers through it
    assert ix.shadow_stats()["builds"] >= 1 and ix.shadow_stats()["rows"] == n, ix.shadow_stats()
    assert ix.remove_ids(("batch", gone)) == gone.size
    fresh = make(np.delete(xb, gone, axis=0))
    ref = fresh.search(xq, k)  # (the fresh index on the coarse filter alone)
    fresh.set_option("flat_shadow", 1)
    for rep in range(3):
        a, b = ix.search(xq, k), fresh.search(xq, k)
        assert np.array_equal(a[1], b[1]) and np.array_equal(u32(a[0]), u32(b[0])), f"stale derived store? rep {rep}"
        assert np.array_equal(a[1], ref[1]) and np.array_equal(u32(a[0]), u32(ref[0]))
    assert ix.shadow_stats()["rows"] == fresh.shadow_stats()["rows"]
    ix.set_option("prefilter", 0)
    ix.set_option("flat_shadow", 0)
    e = ix.search(xq, k)
    assert np.array_equal(e[1], b[1]) and np.array_equal(u32(e[0]), u32(b[0]))


# ---------------------------------------------------------------------------------------------------------------- PQ, SQ8
def code_index(mf, desc, d, metric, rng_seed=5):
    ix = mf.index_factory(d, desc, metric)
    base = desc.split(",")[-1]
    if base.startswith("PQ"):
        M = int(base[2:])
        ix.pq_set_centroids(pqr.synthetic_codebooks(np.random.default_rng(rng_seed), M, d // M))
    else:
        xb = rows_of(d, 1000)
        ix.sq_set_trained(xb.min(axis=0), xb.max(axis=0) - xb.min(axis=0))
    return ix


def codes_of(ix, desc):
    sub = ix.index if desc.startswith("IDMap") else ix
    return sub.pq_codes() if "PQ" in desc else sub.sq_codes()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("desc,d", [("PQ8", 32), ("PQ17", 34), ("SQ8", 5), ("SQ8", 48), ("IDMap,PQ8", 32), ("IDMap,PQ17", 34), ("IDMap,SQ8", 5), ("IDMap,SQ8", 48)])
def test_code_stores(mf, desc, d, metric):
    n = 1000
    xb = rows_of(d, n)
    mapped = desc.startswith("IDMap")
    ext = (np.arange(n, dtype=np.int64) * 5 + 2) % 811 if mapped else np.arange(n, dtype=np.int64)
    gone = np.unique(np.concatenate([ext[:17], ext[300:620], ext[::9], ext[-1:]]))  # leading rows, a run beyond a workgroup's tile, the last row
    for kind, sel in selectors(gone, int(ext.max())).items():
        ix = code_index(mf, desc, d, metric)
        ix.add_with_ids(xb, ext) if mapped else ix.add(xb)
        before = codes_of(ix, desc)
        keep = rr.stable_keep(ext, sel)
        assert ix.remove_ids(sel) == n - keep.size and ix.ntotal == keep.size
        assert np.array_equal(codes_of(ix, desc), before[keep]), f"{desc} {kind}: codes"
        fresh = code_index(mf, desc, d, metric)
        fresh.add_with_ids(xb[keep], ext[keep]) if mapped else fresh.add(xb[keep])
        assert_same_answers(ix, fresh, d, False, f"{desc} d {d} {kind}")
        ix.add_with_ids(xb[:50], ext[:50]) if mapped else ix.add(xb[:50])  # add after removal
        fresh.add_with_ids(xb[:50], ext[:50]) if mapped else fresh.add(xb[:50])
        assert_same_answers(ix, fresh, d, False, f"{desc} add after removal", ks=(10,))
        assert np.array_equal(codes_of(ix.clone_to_gpu(0), desc), codes_of(fresh, desc))


# ---------------------------------------------------------------------------------------------------------------- IVF
IVF_D, IVF_N, NLIST = 16, 2000, 16


@functools.lru_cache(maxsize=None)
def ivf_data(metric=L2):
    """rows on an integer lattice (duplicates: list order decides ties); centroids such that, under L2, one list stays empty (a centroid far
    away) and one holds exactly one row"""
    xb = rows_of(IVF_D, IVF_N, lattice=True).copy()
    rng = np.random.default_rng(99)
    cent = (rng.random((NLIST, IVF_D), dtype=np.float32) * 2 - 1).astype(np.float32)
    if metric == L2:
        cent[3] = 100.0  # no row comes near
        cent[9] = -40.0
    xb[777] = -40.0  # under L2 the only row of list 9
    xb.setflags(write=False)
    cent.setflags(write=False)
    return xb, cent


def ivf_index(mf, desc, metric):
    xb, cent = ivf_data(metric)
    ix = mf.index_factory(IVF_D, desc, metric)
    if "_HNSW" in desc:
        ix.train(xb)  # (its quantiser graph is its own: image check only)
    else:
        ix.ivf_set_centroids(cent)
    base = desc.split(",")[-1]
    if base.startswith("PQ"):
        ix.pq_set_centroids(pqr.synthetic_codebooks(np.random.default_rng(5), 8, IVF_D // 8))
    elif base == "SQ8":
        ix.sq_set_trained(np.full(IVF_D, -3, np.float32), np.full(IVF_D, 6, np.float32))
    return ix


def ivf_gone(list_ids, all_ids):
    """a third of the ids, the first and the last one, and EVERY id of the smallest list that holds at least two rows (emptied by the removal)"""
    rng = np.random.default_rng(3)
    all_ids = np.asarray(all_ids, dtype=np.int64)
    sizes = [len(l) for l in list_ids]
    victim = min((s, l) for l, s in enumerate(sizes) if s >= 2)[1]
    return np.unique(np.concatenate([all_ids[rng.random(all_ids.size) < 0.33], all_ids[:1], all_ids[-1:], np.asarray(list_ids[victim], dtype=np.int64)])), victim


IVF_MODES = ["bare", "with_ids", "idmap"]


def ivf_fill(ix, mode):
    """-> (id every row was added with: the stored id, or under IDMap the external id)"""
    xb, _ = ivf_data()
    n = xb.shape[0]
    if mode == "bare":
        ix.add(xb)
        return np.arange(n, dtype=np.int64)
    ids = np.arange(n, dtype=np.int64) * 5 + 3 if mode == "with_ids" else (np.arange(n, dtype=np.int64) * 7 + 1) % 1801  # IDMap: duplicates
    ix.add_with_ids(xb, ids)
    return ids


@pytest.mark.parametrize("mode", IVF_MODES)
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("base", ["IVF16,Flat", "IVF16_HNSW8,Flat"])
def test_ivf_flat(mf, tmp_path, base, metric, mode):
    desc = ("IDMap," if mode == "idmap" else "") + base
    xb, cent = ivf_data(metric)
    ix = ivf_index(mf, desc, metric)
    ids = ivf_fill(ix, mode)
    before = image_of(mf, ix, tmp_path)
    lists = (before["sub"] if mode == "idmap" else before)["lists"]
    if metric == L2 and "_HNSW" not in base:
        assert len(lists[3][0]) == 0 and len(lists[9][0]) == 1
    if mode == "idmap":
        gone, victim = ivf_gone([ids[l[0]] for l in lists], ids)
    else:
        gone, victim = ivf_gone([l[0] for l in lists], ids)
    for kind, sel in selectors(gone, int(ids.max())).items():
        ix = ivf_index(mf, desc, metric)
        ivf_fill(ix, mode)
        if "_HNSW" in base:
            before = image_of(mf, ix, tmp_path)  # (this index's own quantiser)
        want, removed = rr.remove_image(before, sel)
        assert removed == int(np.isin(ids, gone).sum())
        if "_HNSW" not in base:
            assert len((want["sub"] if mode == "idmap" else want)["lists"][victim][0]) == 0  # a list emptied by the removal
        assert ix.remove_ids(sel) == removed and ix.ntotal == xb.shape[0] - removed
        after = image_of(mf, ix, tmp_path, "b.index")
        assert rr.same_image(after, want), f"{desc} {kind}: the image differs from the model"
        if "_HNSW" in base:
            continue
        rows, stored, labels = rr.survivors(want)
        fresh = mf.index_factory(IVF_D, desc, metric)
        fresh.ivf_set_centroids(cent)
        fresh.add_with_ids(rows, labels if mode == "idmap" else stored)
        if mode == "idmap":
            # equal distances come out by STORED id, and a fresh IDMap index numbers its stored ids by arrival: it agrees up to ties.  The
            # index with the contract's stored ids is the model's image, loaded through read_index
            for nprobe in (1, 4, 16):
                assert_same_up_to_ties(ix, fresh, IVF_D, f"{desc} {kind} nprobe {nprobe} (fresh)", nprobe=nprobe)
            p = str(tmp_path / "model.index")
            with open(p, "wb") as f:
                f.write(ff.dumps(want))
            fresh = mf.read_index(p)
        for nprobe in (1, 4, 16):
            assert_same_answers(ix, fresh, IVF_D, True, f"{desc} {kind} nprobe {nprobe}", nprobe=nprobe)
        keep = ("batch", (labels if mode == "idmap" else stored)[::2])
        a, b = ix.search(queries_of(IVF_D, 33), 10, nprobe=4, sel=keep), fresh.search(queries_of(IVF_D, 33), 10, nprobe=4, sel=keep)
        assert np.array_equal(a[1], b[1]) and np.array_equal(u32(a[0]), u32(b[0]))
        # add after removal, then the file and the clone
        ix.add_with_ids(xb[:100], np.arange(100, dtype=np.int64) + 50_000)
        fresh.add_with_ids(xb[:100], np.arange(100, dtype=np.int64) + 50_000)
        assert_same_answers(ix, fresh, IVF_D, True, f"{desc} add after removal", ks=(10,), nprobe=4)
        p = str(tmp_path / "c.index")
        mf.write_index(ix, p)
        assert_same_answers(mf.read_index(p), fresh, IVF_D, False, f"{desc} read_index", ks=(10,), nprobe=4)
        assert_same_answers(ix.clone_to_gpu(0), fresh, IVF_D, False, f"{desc} clone", ks=(10,), nprobe=4)


@pytest.mark.parametrize("mode", IVF_MODES)
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("base", ["IVF16,PQ8", "IVF16,SQ8"])
def test_ivf_coded(mf, base, metric, mode):
    desc = ("IDMap," if mode == "idmap" else "") + base
    xb, cent = ivf_data(metric)
    get = (lambda i, l: i.ivfpq_list(l)) if "PQ" in base else (lambda i, l: i.ivfsq_list(l))
    ix = ivf_index(mf, desc, metric)
    ids = ivf_fill(ix, mode)
    lists = [get(ix, l) for l in range(NLIST)]
    if metric == L2:
        assert len(lists[3][0]) == 0 and len(lists[9][0]) == 1
    gone, victim = ivf_gone([ids[l[0]] if mode == "idmap" else l[0] for l in lists], ids)
    for kind, sel in selectors(gone, int(ids.max())).items():
        ix = ivf_index(mf, desc, metric)
        ivf_fill(ix, mode)
        orders, new_ids, removed, keep_by_id = rr.remove_lists([l[0] for l in lists], sel, ids if mode == "idmap" else None)
        assert removed == int(np.isin(ids, gone).sum()) and orders[victim].size == 0
        assert ix.remove_ids(sel) == removed and ix.ntotal == xb.shape[0] - removed
        for l in range(NLIST):
            gi, gc = get(ix, l)
            assert np.array_equal(gi, new_ids[l]), f"{desc} {kind}: ids of list {l}"
            assert np.array_equal(gc, lists[l][1][orders[l]]), f"{desc} {kind}: codes of list {l}"
        # the fresh index: the surviving rows list by list.  The row a stored id names: bare / IDMap the arrival number, with_ids (id - 3) / 5
        old_stored = np.concatenate([lists[l][0][orders[l]] for l in range(NLIST)])
        src = (old_stored - 3) // 5 if mode == "with_ids" else old_stored
        fresh = ivf_index(mf, desc, metric)
        fresh.add_with_ids(xb[src], ids[old_stored] if mode == "idmap" else old_stored)
        for nprobe in (1, 4, 16):
            assert_same_answers(ix, fresh, IVF_D, False, f"{desc} {kind} nprobe {nprobe}", nprobe=nprobe)
        ix.add_with_ids(xb[:100], np.arange(100, dtype=np.int64) + 50_000)
        fresh.add_with_ids(xb[:100], np.arange(100, dtype=np.int64) + 50_000)
        assert_same_answers(ix, fresh, IVF_D, False, f"{desc} add after removal", ks=(10,), nprobe=4)
        assert_same_answers(ix.clone_to_gpu(0), fresh, IVF_D, False, f"{desc} clone", ks=(10,), nprobe=4)


def test_ivf_edges(mf):
    xb, cent = ivf_data()
    ix = mf.index_factory(IVF_D, "IVF16,Flat", L2)
    assert ix.remove_ids(("batch", [1, 2])) == 0  # untrained and empty
    ix.ivf_set_centroids(cent)
    assert ix.remove_ids(("batch", [1, 2])) == 0 and ix.is_trained
    ix.add(xb)
    assert ix.remove_ids(("batch", [-1, 10**9])) == 0 and ix.ntotal == IVF_N  # no member
    assert ix.remove_ids(("bitmap", np.full(IVF_N // 8, 255, np.uint8))) == IVF_N and ix.ntotal == 0 and ix.is_trained
    ix.add(xb[:300])  # numbered from the new ntotal
    fresh = mf.index_factory(IVF_D, "IVF16,Flat", L2)
    fresh.ivf_set_centroids(cent)
    fresh.add(xb[:300])
    assert_same_answers(ix, fresh, IVF_D, True, "IVF refilled after removing every row", nprobe=16)


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("desc", ["HNSW16", "HNSW16,SQ8", "IVF16,PQ8,RFlat", "IDMap,HNSW16", "sharded"])
def test_refusals_leave_the_index_alone(mf, desc):
    d, n = 16, 600
    xb = rows_of(d, n, lattice=True)
    if desc == "sharded":
        ix = mf.index_factory(d, "Flat", L2)
        ix.add(xb)
        ix.shard_to_gpus([0, 0])
    else:
        ix = mf.index_factory(d, desc, L2)
        if "RFlat" in desc:
            ix.refine_base.ivf_set_centroids(ivf_data()[1])
            ix.refine_base.pq_set_centroids(pqr.synthetic_codebooks(np.random.default_rng(5), 8, d // 8))
        elif not ix.is_trained:
            ix.train(xb)
        ix.add_with_ids(xb, np.arange(n, dtype=np.int64)) if desc.startswith("IDMap") else ix.add(xb)
    xq = queries_of(d, 7)
    D0, I0 = ix.search(xq, 10)
    for sel in selectors(np.arange(0, n, 2), n).values():
        with pytest.raises(mf.FaissException) as e:
            ix.remove_ids(sel)
        assert TEXT in str(e.value)
    assert ix.ntotal == n
    D1, I1 = ix.search(xq, 10)
    assert np.array_equal(I0, I1) and np.array_equal(u32(D0), u32(D1))


def test_selector_none_is_an_error(mf):
    ix = mf.index_factory(8, "Flat", L2)
    ix.add(rows_of(8, 100))
    assert mf.lib().mvs_index_remove_ids(ix._h, 0, None, 0, None) != 0
    assert "selector kind 0" in mf.lib().mvs_last_error().decode()
    assert mf.lib().mvs_index_remove_ids(ix._h, 9, None, 0, None) != 0
    assert mf.lib().mvs_index_remove_ids(ix._h, 2, None, 0, None) == 0 and ix.ntotal == 100  # an empty batch; n_removed may be null


# ---------------------------------------------------------------------------------------------------------------- adaptor and driver
@pytest.mark.parametrize("desc", ["IDMap,Flat", "Flat", "IDMap,IVF16,Flat"])
def test_boundary_driver_remove(desc):
    """the compat faiss::Index::remove_ids (IDSelectorBatch, then IDSelectorBitmap) through host/boundary_driver: counts, ntotal on the
    wrapper chain and on the handles, a search against a fresh index"""
    exe = os.path.join(ROOT, "duckdb-faiss-ext_amd", "host", "boundary_driver")
    r = subprocess.run([exe, "remove", "3000", "24", "33", desc], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and "REMOVE OK 1000 500 1500" in r.stdout, r.stdout[-2000:]
