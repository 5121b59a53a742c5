"""PQ<M> / IDMap,PQ<M> on the device against the CPU model of tests/pq_reference.py: every comparison is bitwise (labels
array_equal, distances as uint32).  Where training is not under test both sides use the same codebooks through pq_set_centroids,
so a k-means mismatch cannot mask a scan bug."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import pq_reference as pqr
from helpers import bitmap_from_ids
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "duckdb-faiss-ext_amd", "host", "boundary_driver")
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
TRAIN_SHAPES = [(8, 2), (3, 3), (12, 4), (64, 4), (96, 4)]  # dsub 4, 1, 3, 16, 24


def _mf():
    import mi355_faiss as mf

    return mf


def _same(D, I, Dr, Ir, what):
    assert np.array_equal(I, Ir), f"{what}: labels differ in {(I != Ir).sum()} slots, first query {np.argwhere(I != Ir)[0][0]}"
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32)), f"{what}: distances differ in {(D != Dr).sum()} slots"


@functools.lru_cache(maxsize=None)
def _trained(d, M):
    """(training rows, reference codebooks) -- computed once, shared by the training and the encode tests"""
    rng = np.random.default_rng(100 * d + M)
    x = rng.standard_normal((2000, d)).astype(np.float32)
    x[rng.integers(0, 2000, 100)] = x[rng.integers(0, 2000, 100)]  # repeated rows: equal distances inside the k-means
    cb = pqr.train_codebooks(x, M)
    x.setflags(write=False)
    cb.setflags(write=False)
    return x, cb


# ------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("d,M", TRAIN_SHAPES)
def test_train_gives_the_reference_codebooks(d, M):
    mf = _mf()
    x, cb = _trained(d, M)
    ix = mf.index_factory(d, f"PQ{M}", L2)
    assert not ix.is_trained and ix.pq_info() == (M, 8)
    ix.train(x)
    assert ix.is_trained
    assert np.array_equal(ix.pq_centroids().view(np.uint32), cb.view(np.uint32))


def test_train_under_inner_product_is_l2_kmeans_and_can_be_repeated_while_empty():
    mf = _mf()
    x, cb = _trained(8, 2)
    ix = mf.index_factory(8, "PQ2", IP)
    ix.train(x[:1000])
    ix.train(x)  # ntotal == 0: retrains, as FAISS does
    assert np.array_equal(ix.pq_centroids().view(np.uint32), cb.view(np.uint32))
    ix.add(x[:5])
    with pytest.raises(mf.FaissException, match="only possible while it is empty"):
        ix.train(x)


def test_train_needs_256_rows_and_add_needs_training():
    mf = _mf()
    x, _ = _trained(8, 2)
    for desc in ("PQ2", "IDMap,PQ2"):
        ix = mf.index_factory(8, desc, L2)
        with pytest.raises(mf.FaissException, match="at least as large as number of clusters"):
            ix.train(x[:255])
        assert not ix.is_trained
        with pytest.raises(mf.FaissException, match="is_trained"):
            ix.add(x[:10]) if desc == "PQ2" else ix.add_with_ids(x[:10], np.arange(10))
        assert ix.ntotal == 0


# ------------------------------------------------------------------------------------------------ encode
@pytest.mark.parametrize("d,M", TRAIN_SHAPES + [(160, 2)])  # (160, 2): dsub 80, the codebook is read through the caches
def test_codes_equal_the_reference_whatever_the_batches(d, M):
    mf = _mf()
    rng = np.random.default_rng(7 * d + M)
    if (d, M) in TRAIN_SHAPES:
        x, cb = _trained(d, M)
    else:
        cb = pqr.synthetic_codebooks(rng, M, d // M)
    xb = rng.standard_normal((6000, d)).astype(np.float32)
    xb[:300] = cb[:, rng.integers(0, 256, 300)].transpose(1, 0, 2).reshape(300, d)  # rows ON centroids (also duplicated ones)
    ix = mf.index_factory(d, f"PQ{M}", L2)
    ix.pq_set_centroids(cb)
    assert ix.is_trained
    i0 = 0
    for n in (1, 19, 20, 1000, 6000 - 1040):  # 1 + 19 + 20 + 1000 + rest: batch independence, growth of the code store
        ix.add(xb[i0 : i0 + n])
        i0 += n
    assert ix.ntotal == 6000
    ref = pqr.encode(cb, xb)
    assert np.array_equal(ix.pq_codes(), ref)
    assert np.array_equal(ix.pq_codes(4000, 100), ref[4000:4100])


# ------------------------------------------------------------------------------------------------ search
SEARCH_SHAPES = [(1, 8), (2, 1), (3, 4), (8, 8), (16, 4), (33, 1), (64, 4), (128, 1)]  # (M, dsub): float4 x5, float2 x2, scalar


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("M,dsub", SEARCH_SHAPES)
def test_search_is_the_pure_order_of_the_reference_sums(metric, M, dsub):
    mf = _mf()
    d = M * dsub
    rng = np.random.default_rng(1000 * M + dsub + metric)
    cb = pqr.synthetic_codebooks(rng, M, dsub)
    ix = mf.index_factory(d, f"PQ{M}", metric)
    ix.pq_set_centroids(cb)
    Q, R = ix.get_stat("pq_query_block"), ix.get_stat("pq_rows_per_workgroup")
    assert Q >= 1 and R >= 64
    nmax, nqmax = 2 * R + 3, 2 * Q + 1
    xb = rng.standard_normal((nmax, d)).astype(np.float32)
    xb[rng.integers(0, nmax, nmax // 8)] = xb[rng.integers(0, nmax, nmax // 8)]  # duplicate rows -> tied sums
    xq = rng.standard_normal((nqmax, d)).astype(np.float32)
    codes = pqr.encode(cb, xb)
    dis = pqr.distances(pqr.tables(cb, xq, metric), codes)  # [nqmax, nmax], computed once; every case below is a slice of it
    nqs, ks = [1, Q - 1, Q, Q + 1, 2 * Q + 1], [1, 10, 100, 1000]
    nqs = [v for v in nqs if v >= 1]
    have = 0
    for i, n in enumerate([1, 63, 64, 65, R - 1, R, R + 1, 2 * R + 3]):
        ix.add(xb[have:n])
        have = n
        if i == 0:
            assert np.array_equal(ix.pq_codes(), codes[:1])
        cases = [(nqs[i % len(nqs)], ks[i % 4]), (nqs[(i + 2) % len(nqs)], ks[(i + 1) % 4])]
        if n == nmax:
            cases = [(nq, 10) for nq in nqs] + [(Q + 1, k) for k in ks]
        for nq, k in cases:
            D, I = ix.search(xq[:nq], k)
            Dr, Ir = pqr.select(dis[:nq, :n], k, metric)
            _same(D, I, Dr, Ir, f"M={M} n={n} nq={nq} k={k}")
            if k > n:
                assert (I[:, n:] == -1).all() and (D[:, n:] == (pqr.FLT_MAX if metric == L2 else -pqr.FLT_MAX)).all()
    assert np.array_equal(ix.pq_codes(), codes)
    assert ix.last_kernel_info()["name"] == "pq_scan_kernel"
    with pytest.raises(mf.FaissException, match="2048"):
        ix.search(xq[:1], 2049)
    D, I = ix.search(xq[:2], 2048)
    _same(D, I, *pqr.select(dis[:2], 2048, metric), f"M={M} k=2048")


@pytest.mark.parametrize("metric", [L2, IP])
def test_one_subquantizer_has_ties_at_every_boundary(metric):
    mf = _mf()
    rng = np.random.default_rng(11 + metric)
    cb = pqr.synthetic_codebooks(rng, 1, 4)
    xb = rng.standard_normal((3000, 4)).astype(np.float32)
    xq = rng.standard_normal((9, 4)).astype(np.float32)
    ix = mf.index_factory(4, "PQ1", metric)
    ix.pq_set_centroids(cb)
    ix.add(xb)
    dis = pqr.distances(pqr.tables(cb, xq, metric), pqr.encode(cb, xb))
    assert max(len(np.unique(row)) for row in dis) <= 256
    for k in (1, 10, 100, 1000):
        D, I = ix.search(xq, k)
        _same(D, I, *pqr.select(dis, k, metric), f"PQ1 k={k}")


@pytest.mark.parametrize("edge_in_R", [1, 2, 3])  # workgroup edges are at multiples of R; 3R is also where a row range ends
def test_copies_of_one_row_across_a_workgroup_edge_keep_the_lowest_rows(edge_in_R):
    mf = _mf()
    rng = np.random.default_rng(edge_in_R)
    cb = pqr.synthetic_codebooks(rng, 8, 2)
    ix = mf.index_factory(16, "PQ8", L2)
    ix.pq_set_centroids(cb)
    R = ix.get_stat("pq_rows_per_workgroup")
    edge = edge_in_R * R
    xb = rng.standard_normal((edge + 400, 16)).astype(np.float32)
    xq = rng.standard_normal((5, 16)).astype(np.float32)
    xb[edge - 250 : edge + 250] = xq[0]  # 500 copies of the first query itself: its best rows, all tied
    ix.add(xb)
    D, I = ix.search(xq, 10)
    assert I[0].tolist() == list(range(edge - 250, edge - 240))
    _same(D, I, *pqr.search(cb, pqr.encode(cb, xb), xq, 10, L2), f"copies across row {edge}")


def test_rows_arriving_best_last_overflow_the_buckets_and_are_rescanned(tmp_path):
    """codes written through a file so that the sums DEcrease with the row number: every row of a range beats the bound"""
    mf = _mf()
    probe = mf.index_factory(2, "PQ2", L2)
    R = probe.get_stat("pq_rows_per_workgroup")
    n = 3 * R + 5
    assert n <= 65536
    cb = np.zeros((2, 256, 1), dtype=np.float32)
    cb[0, :, 0] = 256.0 * np.arange(256)
    cb[1, :, 0] = np.arange(256)
    codes = np.stack([np.arange(n) // 256, np.arange(n) % 256], axis=1).astype(np.uint8)
    path = str(tmp_path / "descending.index")
    pqr.write_pq(path, 2, L2, cb, codes)
    ix = mf.read_index(path)
    xq = np.array([[256.0 * 300, 300.0], [0.0, 0.0], [256.0 * 40 + 7, 3.0]], dtype=np.float32)
    for k in (1, 10, 1000):
        D, I = ix.search(xq, k)
        _same(D, I, *pqr.search(cb, codes, xq, k, L2), f"descending sums k={k}")
        assert I[0, 0] == n - 1
        assert ix.get_stat("pq_scan_rescans") >= 1


# ------------------------------------------------------------------------------------------------ IDMap, selectors
@pytest.mark.parametrize("metric", [L2, IP])
def test_idmap_labels_and_selectors(metric):
    mf = _mf()
    rng = np.random.default_rng(21 + metric)
    n, d, M = 3000, 32, 8
    cb = pqr.synthetic_codebooks(rng, M, d // M)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xb[rng.integers(0, n, 400)] = xb[rng.integers(0, n, 400)]
    xq = rng.standard_normal((11, d)).astype(np.float32)
    ids = rng.permutation(3 * n)[:n].astype(np.int64)
    ix = mf.index_factory(d, "IDMap,PQ8", metric)
    assert ix.kind == mf.KIND_IDMAP and ix.index.kind == mf.KIND_PQ and not ix.is_trained
    ix.pq_set_centroids(cb)
    assert ix.is_trained
    with pytest.raises(mf.FaissException, match="add does not make sense"):
        ix.add(xb[:3])
    ix.add_with_ids(xb[:1000], ids[:1000])
    ix.add_with_ids(xb[1000:], ids[1000:])
    codes = pqr.encode(cb, xb)
    assert np.array_equal(ix.pq_codes(), codes)
    dis = pqr.distances(pqr.tables(cb, xq, metric), codes)
    D, I = ix.search(xq, 10)
    _same(D, I, *pqr.select(dis, 10, metric, labels=ids), "IDMap, no selector")
    keep = ids % 3 == 0
    for k in (10, 1500):  # 1500 > the rows the selector keeps: padded
        Dr, Ir = pqr.select(dis, k, metric, labels=ids, keep=keep)
        D, I = ix.search(xq, k, sel=("bitmap", bitmap_from_ids(ids, keep)))
        _same(D, I, Dr, Ir, f"bitmap k={k}")
        D, I = ix.search(xq, k, sel=("batch", ids[keep]))
        _same(D, I, Dr, Ir, f"batch k={k}")
    D, I = ix.search(xq, 10, sel=("batch", np.array([3 * n + 5], dtype=np.int64)))
    assert (I == -1).all() and (D == (pqr.FLT_MAX if metric == L2 else -pqr.FLT_MAX)).all()
    # a bare PQ index: the selector tests the row number, add_with_ids is FAISS's refusal
    bare = mf.index_factory(d, "PQ8", metric)
    bare.pq_set_centroids(cb)
    with pytest.raises(mf.FaissException, match="add_with_ids not implemented for this type of index"):
        bare.add_with_ids(xb[:3], ids[:3])
    bare.add(xb)
    rows_kept = np.arange(n) % 3 == 0
    D, I = bare.search(xq, 10, sel=("batch", np.arange(n)[rows_kept]))
    _same(D, I, *pqr.select(dis, 10, metric, keep=rows_kept), "bare PQ8, batch selector")


# ------------------------------------------------------------------------------------------------ factory
def test_factory_strings_and_refusals():
    mf = _mf()
    rng = np.random.default_rng(3)
    cb = pqr.synthetic_codebooks(rng, 8, 1)
    xb = rng.standard_normal((500, 8)).astype(np.float32)
    a, b = mf.index_factory(8, "PQ8", L2), mf.index_factory(8, "PQ8x8", L2)
    for ix in (a, b):
        assert ix.kind == mf.KIND_PQ == 5 and ix.pq_info() == (8, 8)
        ix.pq_set_centroids(cb)
        ix.add(xb)
    Da, Ia = a.search(xb[:7], 10)
    Db, Ib = b.search(xb[:7], 10)
    _same(Da, Ia, Db, Ib, "PQ8x8 vs PQ8")
    assert mf.index_factory(8, "IDMap,PQ4", L2).index.kind == 5
    assert mf.index_factory(8, "IDMap2,PQ4", IP).index.pq_info() == (4, 8)
    assert mf.index_factory(256, "PQ128", L2).pq_info() == (128, 8)
    with pytest.raises(mf.FaissException, match="This index type is not implemented on the MI355X path yet: PQ8x4"):
        mf.index_factory(8, "PQ8x4", L2)
    with pytest.raises(mf.FaissException, match="This index type is not implemented on the MI355X path yet: PQ256.*128"):
        mf.index_factory(256, "PQ256", L2)
    with pytest.raises(mf.FaissException, match="multiple of the number of subquantizers"):
        mf.index_factory(8, "PQ5", L2)
    with pytest.raises(mf.FaissException, match="metric type 2 is not implemented on the MI355X path"):
        mf.index_factory(8, "PQ8", 2)
    with pytest.raises(mf.FaissException, match="could not parse index string"):
        mf.index_factory(8, "PQ", L2)
    with pytest.raises(mf.FaissException, match="not a PQ index"):
        mf.index_factory(8, "Flat", L2).pq_info()


# ------------------------------------------------------------------------------------------------ persistence, placement
@pytest.mark.parametrize("desc", ["PQ4", "IDMap,PQ4"])
def test_write_read_clone_and_the_python_written_file(desc, tmp_path):
    mf = _mf()
    rng = np.random.default_rng(31)
    n, d, M = 2500, 12, 4
    cb = pqr.synthetic_codebooks(rng, M, d // M)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((9, d)).astype(np.float32)
    ids = (rng.permutation(10 * n)[:n]).astype(np.int64) if desc.startswith("IDMap") else None
    ix = mf.index_factory(d, desc, IP)
    ix.pq_set_centroids(cb)
    ix.add(xb) if ids is None else ix.add_with_ids(xb, ids)
    codes = pqr.encode(cb, xb)
    Dr, Ir = pqr.search(cb, codes, xq, 20, IP, labels=ids)
    _same(*ix.search(xq, 20), Dr, Ir, desc)
    # write -> the Python parser sees the same index; read_index searches identically
    path = str(tmp_path / "a.index")
    mf.write_index(ix, path)
    img = pqr.parse_pq(path)
    assert (img["d"], img["ntotal"], img["M"], img["nbits"], img["metric"], img["trained"]) == (d, n, M, 8, IP, True)
    assert (img["search_type"], img["encode_signs"], img["polysemous_ht"]) == (0, 0, 8 * M + 1)
    assert np.array_equal(img["centroids"].view(np.uint32), cb.view(np.uint32)) and np.array_equal(img["codes"], codes)
    assert (img["ids"] is None) if ids is None else np.array_equal(img["ids"], ids)
    assert open(path, "rb").read() == pqr.write_pq(None, d, IP, cb, codes, ids=ids)
    back = mf.read_index(path)
    assert back.ntotal == n and back.is_trained and back.pq_info() == (M, 8)
    _same(*back.search(xq, 20), Dr, Ir, desc + " after read_index")
    # a Python-written file loads and searches identically
    path2 = str(tmp_path / "b.index")
    pqr.write_pq(path2, d, IP, cb, codes, ids=ids)
    _same(*mf.read_index(path2).search(xq, 20), Dr, Ir, desc + " from a Python-written file")
    # clone_to_gpu(0): an independent copy; to_gpu(0) in place
    clone = ix.clone_to_gpu(0)
    extra = rng.standard_normal((10, d)).astype(np.float32)
    ix.add(extra) if ids is None else ix.add_with_ids(extra, np.arange(10) + 10**6)
    assert clone.ntotal == n and ix.ntotal == n + 10
    _same(*clone.search(xq, 20), Dr, Ir, desc + " clone")
    clone.to_gpu(0)
    _same(*clone.search(xq, 20), Dr, Ir, desc + " clone after to_gpu")
    # an untrained, empty index round-trips too
    path3 = str(tmp_path / "c.index")
    mf.write_index(mf.index_factory(d, desc, L2), path3)
    empty = mf.read_index(path3)
    assert not empty.is_trained and empty.ntotal == 0 and empty.pq_info() == (M, 8)


def test_sharding_is_refused():
    mf = _mf()
    rng = np.random.default_rng(41)
    cb = pqr.synthetic_codebooks(rng, 4, 2)
    xb = rng.standard_normal((300, 8)).astype(np.float32)
    for desc in ("PQ4", "IDMap,PQ4"):
        ix = mf.index_factory(8, desc, L2)
        ix.pq_set_centroids(cb)
        ix.add(xb) if desc == "PQ4" else ix.add_with_ids(xb, np.arange(300) * 2)
        before = ix.search(xb[:4], 5)
        with pytest.raises(mf.FaissException, match="This index type is not implemented"):
            ix.shard_to_gpus([0, 0])
        with pytest.raises(mf.FaissException, match="This index type is not implemented"):
            ix.clone_to_gpu(-1)
        assert ix.shard_info() is None and ix.ntotal == 300
        _same(*ix.search(xb[:4], 5), *before, desc + " after the refused sharding")


def test_sharded_factory_is_refused():
    """env MVS_DEVICES at creation: a fresh process, as the variable is read when the index is made"""
    code = (
        "import sys; sys.path.insert(0, %r); import mi355_faiss as mf\n"
        "try:\n    mf.index_factory(8, 'IDMap,PQ4', 1)\nexcept mf.FaissException as e:\n    print('REFUSED', e)\n"
    ) % os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, MVS_DEVICES="0,0"))
    assert out.returncode == 0, out.stderr
    assert "REFUSED" in out.stdout and "This index type is not implemented" in out.stdout


# ------------------------------------------------------------------------------------------------ the glue's cast (:704)
def test_idmap_pq_through_the_cpp_glue_path():
    """boundary_driver ingest: CreateFunction, chunked AddFunction from two threads (buffered: the index needs training),
    AddFinaliseFunction (train + add), then a search whose parameters come from innerCreateSearchParameters -- the
    dynamic_cast<faiss::IndexPQ *> under the IndexIDMap"""
    out = subprocess.run([DRIVER, "ingest", "3000", "8", "2", "IDMap,PQ4"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ingest\tOK ntotal=3000" in out.stdout
