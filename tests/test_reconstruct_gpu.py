"""reconstruct, reconstruct_n, reconstruct_batch and search_and_reconstruct on the device (include/mi355_faiss.h "reconstruct", DESIGN.md
3.13).  Every comparison is BITWISE: the rows the device hands back, as uint32, against tests/reconstruct_reference.py applied to the image
write_index produces from the same index.  Shapes are the smallest at which a vectorised row copy can go wrong: d on both sides of a
multiple of 4, of the Flat store's pitches and of 128; dsub = 1; PQ codebooks that fit LDS and that do not; more rows than one workgroup
takes; both sides of bit 4 of the row number (the pair-interleaved Flat layout)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import pq_reference as pqr
import reconstruct_reference as rcr
import sq_reference as sqr

pytestmark = pytest.mark.gpu

L2, IP = 1, 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "duckdb-faiss-ext_amd", "host", "boundary_driver")
RANGE_TEXT = "'ni == 0 || (i0 >= 0 && i0 + ni <= ntotal)' failed"
REFUSAL = "reconstruct not implemented for this type of index"


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss as m

    assert m.device_count() >= 1
    return m


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def rows_of(d, n, seed=0):
    rng = np.random.default_rng(31 * d + n + 1000 * seed)
    xb = (rng.random((n, d), dtype=np.float32) - np.float32(0.25)) * np.float32(3.0)
    xb.setflags(write=False)
    return xb


def centroids_of(d, nlist):
    return np.ascontiguousarray(rows_of(d, 64, seed=7)[:nlist])


def prepare(mf, ix, desc, d, xb):
    """centroids, codebooks and ranges set directly (no k-means over a few hundred rows); what cannot be set is trained"""
    target = ix.refine_base if "RFlat" in desc else ix
    m = [p for p in desc.split(",") if p.startswith("IVF")]
    if m and "_HNSW" in m[0]:
        ix.train(xb)
        return
    if m:
        target.ivf_set_centroids(centroids_of(d, int(m[0][3:])))
    pq = [p for p in desc.split(",") if p.startswith("PQ")]
    if pq:
        M = int(pq[0][2:])
        target.pq_set_centroids(pqr.synthetic_codebooks(np.random.default_rng(d), M, d // M))
    if "SQ8" in desc and "HNSW" not in desc:
        lo, hi = xb.min(axis=0) - np.float32(3.0 if m else 0.0), xb.max(axis=0) + np.float32(3.0 if m else 0.0)
        target.sq_set_trained(lo.astype(np.float32), (hi - lo).astype(np.float32))
    elif not ix.is_trained:
        ix.train(xb)


def build(mf, desc, d, metric, xb, ids=None):
    ix = mf.index_factory(d, desc, metric)
    if any(p.startswith("HNSW") for p in desc.split(",")):
        ix.set_option("hnsw_build_waves", 1)
    prepare(mf, ix, desc, d, xb)
    if ids is not None:
        ix.add_with_ids(xb, ids)
    else:
        ix.add(xb)
    return ix


def model_of(mf, ix, tmp_path, name="a.index", of_row=None):
    p = str(tmp_path / name)
    mf.write_index(ix, p)
    return rcr.load(p, of_row=of_row)


def check_against_model(ix, m, keys):
    """the first, the last and a middle key; a batch with repeats; returns the batch's rows"""
    keys = np.asarray(keys, dtype=np.int64)
    for key in (keys[0], keys[-1], keys[keys.size // 2]):
        assert np.array_equal(u32(ix.reconstruct(int(key))), u32(m.reconstruct(key))), key
    rng = np.random.default_rng(keys.size)
    batch = np.concatenate([rng.permutation(keys), keys[:7], keys[-3:]])
    got = ix.reconstruct_batch(batch)
    assert np.array_equal(u32(got), u32(m.reconstruct_batch(batch)))
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. every kind
F32_SQ_KINDS = ["Flat", "HNSW8", "HNSW8,SQ8", "IVF8,Flat", "IVF8_HNSW4,Flat", "SQ8", "IVF8,SQ8", "SQ8,RFlat"]
PQ_KINDS = ["PQ4", "IVF8,PQ4", "IVF8,PQ4,RFlat"]
CASES = [(k, d) for k in F32_SQ_KINDS for d in (1, 3, 8, 33, 100, 128, 130)] + [(k, d) for k in PQ_KINDS for d in (4, 24, 128, 192)]


@pytest.mark.parametrize("wrapped", [False, True], ids=["bare", "IDMap"])
@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("kind,d", CASES)
def test_every_kind(mf, tmp_path, kind, d, metric, wrapped):
    n = 333 if d != 128 else 1500
    xb = rows_of(d, n)
    # under IDMap the external ids are a permutation of 0 .. n-1: reconstruct_n(0, n) needs every key of the range to exist
    ids = np.random.default_rng(d + n).permutation(n).astype(np.int64) if wrapped else None
    ix = build(mf, ("IDMap," if wrapped else "") + kind, d, metric, xb, ids)
    # ("Flat": no search between add and reconstruct -- the rows are still staged)
    got_n = ix.reconstruct_n(0, n)
    decodes_pq = kind in ("PQ4", "IVF8,PQ4")  # (under RFlat the rows come from the refine store)
    if decodes_pq:  # the range decode writes at least as much as the codebooks hold: LDS where they fit in 128 KB
        assert ix.get_stat("recon_pq_lds") == (1 if d <= 128 else 0)
    one = ix.reconstruct(0)
    if decodes_pq:  # one row is less than the codebooks: through L2
        assert ix.get_stat("recon_pq_lds") == 0
    m = model_of(mf, ix, tmp_path)
    assert m.ntotal == n
    assert np.array_equal(u32(got_n), u32(m.reconstruct_n(0, n)))
    assert np.array_equal(u32(one), u32(m.reconstruct(0)))
    check_against_model(ix, m, np.arange(n))
    if kind in ("Flat", "HNSW8", "IVF8,Flat", "IVF8_HNSW4,Flat", "SQ8,RFlat"):  # the f32 row that was added
        assert np.array_equal(u32(got_n), u32(xb if ids is None else xb[np.argsort(ids)]))
    elif "SQ8" in kind:  # a quantised row is near the row that was added (the range is at most 9 wide: a step of 0.036)
        assert np.abs(got_n - (xb if ids is None else xb[np.argsort(ids)])).max() < 0.1


# ---------------------------------------------------------------------------------------------------------------- 2. batch edges
def test_batch_edges(mf, tmp_path):
    d, n = 8, 1000
    xb = rows_of(d, n)
    ix = build(mf, "SQ8", d, L2, xb)
    m = model_of(mf, ix, tmp_path)
    assert ix.reconstruct_batch(np.empty(0, dtype=np.int64)).shape == (0, d)
    assert ix.reconstruct_n(0, 0).shape == (0, d) and ix.reconstruct_n(5000, 0).shape == (0, d)
    assert np.array_equal(u32(ix.reconstruct_batch([999])), u32(m.rows[[999]]))
    keys = np.random.default_rng(1).integers(0, n, 70_000)
    assert np.array_equal(u32(ix.reconstruct_batch(keys)), u32(m.rows[keys]))
    # a batch larger than one staging chunk of rows (8 MB): d = 130, 20 000 keys
    d2 = 130
    ix2 = build(mf, "Flat", d2, L2, rows_of(d2, 400))
    keys = np.random.default_rng(2).integers(0, 400, 20_000)
    assert np.array_equal(u32(ix2.reconstruct_batch(keys)), u32(rows_of(d2, 400)[keys]))
    # an empty index
    e = mf.index_factory(d, "Flat", L2)
    assert e.reconstruct_n(0, 0).shape == (0, d) and e.reconstruct_batch([]).shape == (0, d)
    with pytest.raises(mf.FaissException, match="ni == 0"):
        e.reconstruct(0)
    D, I, R = e.search_and_reconstruct(rows_of(d, 3), 2)
    assert (I == -1).all() and (R.view(np.uint8) == 0xFF).all()


# ---------------------------------------------------------------------------------------------------------------- 3. duplicates, missing keys
@pytest.mark.parametrize("desc,d", [("IVF4,Flat", 6), ("IVF4,PQ2", 6), ("IDMap,Flat", 6), ("IDMap,IVF4,SQ8", 6)])
def test_duplicates_and_missing_keys(mf, tmp_path, desc, d):
    n = 240
    xb = rows_of(d, n)
    ids = (np.arange(n, dtype=np.int64) * 5 + 11) % 400  # 11, 16, ...: repeats once the sequence wraps at 400
    assert np.unique(ids).size < n
    ix = mf.index_factory(d, desc, L2)
    prepare(mf, ix, desc, d, xb)
    ix.add_with_ids(xb[:100], ids[:100])
    ix.add_with_ids(xb[100:], ids[100:])
    of_row = None
    if not desc.startswith("IDMap"):  # duplicates may sit in different lists: the arrival lists say which came last
        of_row, _ = sqr.assign(L2, centroids_of(d, 4), xb)
    m = model_of(mf, ix, tmp_path, of_row=of_row)
    uniq = np.unique(ids)
    got = ix.reconstruct_batch(uniq)
    assert np.array_equal(u32(got), u32(m.reconstruct_batch(uniq)))
    if "Flat" in desc:  # the last added row of every id, bit for bit
        last = {int(v): i for i, v in enumerate(ids)}
        assert np.array_equal(u32(got), u32(xb[[last[int(v)] for v in uniq]]))
    present, missing_a, missing_b = int(ids[3]), 100_003, -5
    assert missing_a not in ids
    with pytest.raises(mf.FaissException) as e:
        ix.reconstruct_batch([present, missing_a, present, missing_b])
    assert "key not found" in str(e.value) and str(missing_a) in str(e.value) and str(missing_b) not in str(e.value)
    with pytest.raises(mf.FaissException, match="key not found"):
        ix.reconstruct(missing_b)
    assert np.array_equal(u32(ix.reconstruct(present)), u32(m.reconstruct(present)))  # (the index still answers)


def test_range_errors_and_untouched_rows(mf):
    d = 5
    xb = rows_of(d, 40)
    flat = build(mf, "Flat", d, L2, xb)
    for bad in (40, -1):
        with pytest.raises(mf.FaissException) as e:
            flat.reconstruct(bad)
        assert RANGE_TEXT in str(e.value)
    with pytest.raises(mf.FaissException) as e:
        flat.reconstruct_n(30, 11)
    assert RANGE_TEXT in str(e.value)
    # bare IVF4,Flat with ids {5, 7, 9}: reconstruct_n(4, 8) writes rows 1, 3 and 5 and leaves the others as they were
    iv = mf.index_factory(d, "IVF4,Flat", L2)
    iv.ivf_set_centroids(centroids_of(d, 4))
    iv.add_with_ids(xb[:3], np.array([5, 7, 9], dtype=np.int64))
    sentinel = np.full((8, d), np.float32(-123.25))
    out = iv.reconstruct_n(4, 8, out=sentinel.copy())
    want = sentinel.copy()
    want[[1, 3, 5]] = xb[:3]
    assert np.array_equal(u32(out), u32(want))


# ---------------------------------------------------------------------------------------------------------------- 4. table lifetime
@pytest.mark.parametrize("desc", ["IDMap,IVF8,Flat", "IVF8,SQ8", "IDMap,Flat", "IDMap,IVF8,PQ4"])
def test_table_lifetime(mf, tmp_path, desc):
    d, n0, n1 = 8, 700, 5000  # (the second add grows every store past its first allocation of 4096 rows)
    xb = rows_of(d, n0 + n1)
    ids = np.arange(n0 + n1, dtype=np.int64) * 3 + 7
    ix = mf.index_factory(d, desc, L2)
    prepare(mf, ix, desc, d, xb)
    ix.add_with_ids(xb[:n0], ids[:n0])
    m0 = model_of(mf, ix, tmp_path, "0.index")
    check_against_model(ix, m0, ids[:n0])
    ix.add_with_ids(xb[n0:], ids[n0:])  # the table is dropped: old and new keys
    m1 = model_of(mf, ix, tmp_path, "1.index")
    check_against_model(ix, m1, ids)
    assert np.array_equal(u32(ix.reconstruct_batch(ids[:n0])), u32(m0.reconstruct_batch(ids[:n0])))
    # half the rows go: survivors reconstruct to the same bits, removed keys raise
    gone, kept = ids[::2], ids[1::2]
    assert ix.remove_ids(("batch", gone)) == gone.size
    assert np.array_equal(u32(ix.reconstruct_batch(kept)), u32(m1.reconstruct_batch(kept)))
    with pytest.raises(mf.FaissException) as e:
        ix.reconstruct_batch([int(kept[0]), int(gone[5]), int(gone[2])])
    assert "key not found" in str(e.value) and str(int(gone[5])) in str(e.value)
    # images and clones
    p = str(tmp_path / "2.index")
    mf.write_index(ix, p)
    for other in (mf.read_index(p), ix.clone_to_gpu(0)):
        assert np.array_equal(u32(other.reconstruct_batch(kept)), u32(m1.reconstruct_batch(kept)))
        with pytest.raises(mf.FaissException, match="key not found"):
            other.reconstruct(int(gone[0]))


# ---------------------------------------------------------------------------------------------------------------- 5. search_and_reconstruct
SAR = [("Flat", {}), ("IDMap,Flat", {}), ("IVF8,Flat", {"nprobe": 4}), ("HNSW8", {"efSearch": 32}), ("IDMap,IVF8,PQ4,RFlat", {"nprobe": 3}),
       ("IDMap,IVF8,SQ8", {"nprobe": 8}), ("HNSW8,SQ8", {"efSearch": 24})]


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("desc,kw", SAR, ids=[s[0] for s in SAR])
def test_search_and_reconstruct(mf, tmp_path, desc, kw, metric):
    import torch

    d, n, k = 24, 600, 10
    xb = rows_of(d, n)
    wrapped = desc.startswith("IDMap")
    ids = np.arange(n, dtype=np.int64) * 3 + 7 if wrapped else None
    ix = build(mf, desc, d, metric, xb, ids)
    if "RFlat" in desc:
        ix.k_factor = 3
    m = model_of(mf, ix, tmp_path)
    labels = ids if wrapped else np.arange(n, dtype=np.int64)
    few = labels[[5, 77, 300]]
    for nq, sel, kk in ((7, None, k), (33, None, k), (7, ("batch", labels[::3]), k), (9, ("batch", few), 5)):
        xq = rows_of(d, nq, seed=3)
        D0, I0 = ix.search(xq, kk, sel=sel, **kw)
        D, I, R = ix.search_and_reconstruct(xq, kk, sel=sel, **kw)
        assert np.array_equal(I, I0) and np.array_equal(u32(D), u32(D0)), (nq, sel is not None)
        assert np.array_equal(u32(R), u32(m.of_labels(I)))
        for q in (0, nq - 1):
            for j in (0, kk - 1):
                if I[q, j] >= 0:
                    assert np.array_equal(u32(R[q, j]), u32(ix.reconstruct(int(I[q, j]))))
        if sel is not None and sel[1] is few:  # k beyond the rows the selector admits: padded slots are rows of 0xFF bytes
            assert (I[:, 3:] == -1).all() and (R[:, 3:].view(np.uint8) == 0xFF).all()
        # the device-resident variant on torch tensors: the same bits
        tq = torch.from_numpy(np.array(xq)).cuda()
        Dt, It, Rt = ix.search_and_reconstruct_torch(tq, kk, sel=sel, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(It.cpu().numpy(), I) and np.array_equal(u32(Dt.cpu().numpy()), u32(D)) and np.array_equal(u32(Rt.cpu().numpy()), u32(R))
    keys = torch.from_numpy(labels[::-1].copy()).cuda()
    Rk = ix.reconstruct_batch_torch(keys)
    assert np.array_equal(u32(Rk.cpu().numpy()), u32(m.reconstruct_batch(labels[::-1])))
    bad = torch.from_numpy(np.array([labels[1], 10**9, labels[2]], dtype=np.int64)).cuda()
    with pytest.raises(mf.FaissException) as e:
        ix.reconstruct_batch_torch(bad)
    assert str(10**9) in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- 6. side effects, refusals
def test_search_is_unchanged_by_a_reconstruction_ivf(mf):
    d, n = 24, 900
    xb = rows_of(d, n)
    ix = build(mf, "IVF8,Flat", d, L2, xb)
    xq = rows_of(d, 33, seed=3)
    D0, I0 = ix.search(xq, 10, nprobe=4)
    ix.reconstruct_batch(np.arange(n)[::-1])
    ix.search_and_reconstruct(xq[:5], 3, nprobe=2)
    D1, I1 = ix.search(xq, 10, nprobe=4)
    assert np.array_equal(I0, I1) and np.array_equal(u32(D0), u32(D1))


def test_search_is_unchanged_by_a_reconstruction_flat_with_its_shadow(mf):
    from oracle import oracle as orc

    d, n, nq, k = 64, 300_000, 600, 10
    xb = orc.synth_clustered(n, d, 7, n_centers=256, sigma=0.05)
    xb = np.round(xb * 8) / 8
    xq = xb[np.random.RandomState(3).randint(0, n, nq)].copy()
    ix = mf.index_factory(d, "Flat", L2)
    ix.add(xb)
    ix.set_option("flat_shadow", 1)
    for _ in range(2):
        D0, I0 = ix.search(xq, k)
    assert "flat shadow" in ix.last_kernel_info()["name"]
    keys = np.random.default_rng(0).integers(0, n, 5000)
    assert np.array_equal(u32(ix.reconstruct_batch(keys)), u32(xb[keys]))
    D1, I1 = ix.search(xq, k)
    assert "flat shadow" in ix.last_kernel_info()["name"] and ix.shadow_stats()["builds"] == 1
    assert np.array_equal(I0, I1) and np.array_equal(u32(D0), u32(D1))


def test_a_sharded_index_refuses_and_stays_searchable(mf):
    import torch

    d, n = 16, 600
    xb = rows_of(d, n)
    ix = build(mf, "Flat", d, L2, xb)
    xq = rows_of(d, 7, seed=3)
    D0, I0 = ix.search(xq, 10)
    ix.shard_to_gpus([0, 0])
    calls = [lambda: ix.reconstruct(3), lambda: ix.reconstruct_n(0, 5), lambda: ix.reconstruct_batch([1, 2]), lambda: ix.search_and_reconstruct(xq, 3),
             lambda: ix.reconstruct_n(0, 0), lambda: ix.reconstruct_batch_torch(torch.arange(4, dtype=torch.int64, device="cuda")),
             lambda: ix.search_and_reconstruct_torch(torch.from_numpy(np.array(xq)).cuda(), 3)]
    for call in calls:
        with pytest.raises(mf.FaissException) as e:
            call()
        assert REFUSAL in str(e.value)
    D1, I1 = ix.search(xq, 10)
    assert np.array_equal(I0, I1) and np.array_equal(u32(D0), u32(D1))


# ---------------------------------------------------------------------------------------------------------------- 7. the faiss:: adaptor
@pytest.mark.parametrize("desc", ["Flat", "IDMap,Flat"])
def test_adaptor_through_the_boundary_driver(desc):
    """faiss::Index::reconstruct, reconstruct_batch, reconstruct_n and search_and_reconstruct of compat/faiss/Index.h, driven by
    host/boundary_driver.cpp's `reconstruct` sub-command"""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    out = subprocess.run([DRIVER, "reconstruct", "120", "24", "5", desc], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RECONSTRUCT OK 120 10" in out.stdout, out.stdout + out.stderr
