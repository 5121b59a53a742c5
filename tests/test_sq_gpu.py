"""SQ8 / IDMap,SQ8 on the device against the CPU model of tests/sq_reference.py: every comparison of codes, labels and distances is
bitwise (labels array_equal, distances as uint32); the trained range is compared as values."""
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


def _index(d, desc, metric, vmin, vdiff):
    ix = _mf().index_factory(d, desc, metric)
    assert not ix.is_trained
    ix.sq_set_trained(vmin, vdiff)
    assert ix.is_trained
    return ix


def _rows(rng, n, d):
    """rows with per-dimension scales and offsets, a few repeated"""
    x = (rng.standard_normal((n, d)) * rng.uniform(0.1, 10, d) + rng.uniform(-5, 5, d)).astype(np.float32)
    m = max(n // 10, 1)
    x[rng.integers(0, n, m)] = x[rng.integers(0, n, m)]
    return x


# ------------------------------------------------------------------------------------------------ training, encoding
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,n", [(1, 1), (5, 513), (64, 70000), (768, 1100)])  # one row; a chunk edge of the reduction; two upload batches
def test_train_gives_the_numpy_range(d, n, metric):
    mf = _mf()
    rng = np.random.default_rng(10 * d + metric)
    x = _rows(rng, n, d)
    x[:, d // 2] = -7.25  # a constant dimension
    ix = mf.index_factory(d, "SQ8", metric)
    assert ix.kind == mf.KIND_SQ == 7 and not ix.is_trained
    if d == 5:
        ix.train(x[:100])  # ntotal == 0: training again is accepted
    ix.train(x)
    assert ix.is_trained
    vmin, vdiff = sqr.train_range(x)
    gmin, gdiff = ix.sq_trained()
    assert (gmin == vmin).all() and (gdiff == vdiff).all() and gdiff[d // 2] == 0
    m = min(n, 3000)
    ix.add(x[:m])
    assert np.array_equal(ix.sq_codes(), sqr.encode(vmin, vdiff, x[:m]))
    with pytest.raises(mf.FaissException, match="only possible while it is empty"):
        ix.train(x)
    with pytest.raises(mf.FaissException, match="only possible while it is empty"):
        ix.sq_set_trained(vmin, vdiff)


def test_training_and_adding_errors():
    mf = _mf()
    x = _rows(np.random.default_rng(1), 50, 8)
    for desc in ("SQ8", "IDMap,SQ8"):
        ix = mf.index_factory(8, desc, L2)
        with pytest.raises(mf.FaissException, match="n > 0"):
            ix.train(x[:0])
        assert not ix.is_trained
        with pytest.raises(mf.FaissException, match="is_trained"):
            ix.add_with_ids(x[:10], np.arange(10)) if desc.startswith("IDMap") else ix.add(x[:10])
        with pytest.raises(mf.FaissException, match="is_trained"):
            ix.search(x[:1], 1)
        assert ix.ntotal == 0
        ix.train(x)
        assert ix.is_trained
    bare = mf.index_factory(8, "SQ8", L2)
    bare.train(x)
    with pytest.raises(mf.FaissException, match="add_with_ids not implemented for this type of index"):
        bare.add_with_ids(x[:10], np.arange(10))
    assert bare.ntotal == 0


@pytest.mark.parametrize("how", ["add", "IDMap"])
def test_codes_equal_the_reference_whatever_the_batches(how):
    rng = np.random.default_rng(17)
    d, n = 19, 6000
    xb = _rows(rng, n, d)
    vmin, vdiff = sqr.train_range(xb[:3000])  # trained on half of the rows: the others fall outside the range here and there
    vdiff[3] = 0.0  # a constant dimension
    xb[5000:5200] *= 3.0  # far outside
    ids = None if how == "add" else rng.permutation(10 * n)[:n].astype(np.int64)
    ix = _index(d, "IDMap,SQ8" if how == "IDMap" else "SQ8", L2, vmin, vdiff)
    i0 = 0
    for m in (1, 2048, 19, 1001, n - 3069):  # batch independence, growth of the code store
        ix.add(xb[i0 : i0 + m]) if ids is None else ix.add_with_ids(xb[i0 : i0 + m], ids[i0 : i0 + m])
        i0 += m
    assert ix.ntotal == n
    codes = sqr.encode(vmin, vdiff, xb)
    assert (codes[:, 3] == 0).all() and (codes == 0).any() and (codes == 255).any()
    assert np.array_equal(ix.sq_codes(), codes)
    assert np.array_equal(ix.sq_codes(2047, 3), codes[2047:2050])
    _same(*ix.search(xb[:7], 10), *sqr.sq_search(L2, vmin, vdiff, codes, xb[:7], 10, labels=ids), how)


# ------------------------------------------------------------------------------------------------ search
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [1, 5, 16, 17, 100, 128, 768, 1536])  # padding of the 16-byte words, every edge of the 32-component chunks
def test_search_equals_the_model(metric, d):
    rng = np.random.default_rng(1000 * d + metric)
    n = 2100  # two staged blocks of 1024 rows and a part of a third
    xb = _rows(rng, n, d)
    vmin, vdiff = sqr.train_range(xb)
    ix = _index(d, "SQ8", metric, vmin, vdiff)
    Q, R = ix.get_stat("sq_pair_block"), ix.get_stat("sq_rows_per_workgroup")
    assert 1 <= Q <= 32 and R >= 1024
    # an empty trained index: every slot is padding
    D, I = ix.search(xb[:3], 5)
    assert (I == -1).all() and (D == (sqr.FLT_MAX if metric == L2 else -sqr.FLT_MAX)).all()
    ix.add(xb[:1500])
    ix.add(xb[1500:])
    codes = sqr.encode(vmin, vdiff, xb)
    assert np.array_equal(ix.sq_codes(), codes)
    xq = np.concatenate([_rows(rng, 2 * Q + 1 - 6, d), xb[:6]])
    dis = sqr.sq_distances(metric, vmin, vdiff, codes, xq)
    for nq, k in ((Q - 1, 1), (Q, 10), (Q + 1, 100), (2 * Q + 1, 2048), (1, 2048)):  # pair groups; k up to the largest; one query
        D, I = ix.search(xq[:nq], k)
        _same(D, I, *sqr.sq_select(dis[:nq], k, metric), f"d={d} nq={nq} k={k}")
    assert ix.last_kernel_info()["name"] == "sq8_scan_kernel"
    # k beyond the rows: -1 padding
    small = _index(d, "SQ8", metric, vmin, vdiff)
    small.add(xb[:37])
    D, I = small.search(xq[:3], 100)
    _same(D, I, *sqr.sq_select(dis[:3, :37], 100, metric), f"d={d} k beyond the rows")
    assert (I[:, 37:] == -1).all()


@pytest.mark.parametrize("metric", [L2, IP])
def test_row_counts_around_the_rows_of_a_workgroup(metric):
    """R - 1, R, R + 1 rows (segment edge) and 3 R + 7 (the windows [0, R), [R, 3 R), [3 R, ...)), grown by adds"""
    d = 5
    rng = np.random.default_rng(30 + metric)
    R = _index(d, "SQ8", metric, np.zeros(d), np.ones(d)).get_stat("sq_rows_per_workgroup")
    n = 3 * R + 7
    assert n <= 40000
    xb = _rows(rng, n, d)
    xq = _rows(rng, 9, d)
    vmin, vdiff = sqr.train_range(xb)
    codes = sqr.encode(vmin, vdiff, xb)
    dis = sqr.sq_distances(metric, vmin, vdiff, codes, xq)
    ix = _index(d, "SQ8", metric, vmin, vdiff)
    have = 0
    for m, k in ((R - 1, 10), (R, 2048), (R + 1, 100), (n, 1000)):
        ix.add(xb[have:m])
        have = m
        _same(*ix.search(xq, k), *sqr.sq_select(dis[:, :m], k, metric), f"{m} rows k={k}")
    assert ix.get_stat("sq_scan_launches") >= 3


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("metric", [L2, IP])
def test_integer_lattice_ties_follow_the_row(metric):
    rng = np.random.default_rng(50 + metric)
    d = 4
    vmin, vdiff = np.full(d, -0.5, dtype=np.float32), np.full(d, 255.0, dtype=np.float32)  # s = 1, a = 0: a code decodes to itself
    xb = rng.integers(0, 7, size=(4000, d)).astype(np.float32)  # 7^4 points: many equal rows
    xb[3000:3500] = xb[2000:2500]
    xq = rng.integers(-4, 12, size=(21, d)).astype(np.float32)
    ix = _index(d, "SQ8", metric, vmin, vdiff)
    ix.add(xb)
    codes = sqr.encode(vmin, vdiff, xb)
    assert np.array_equal(codes.astype(np.float32), xb) and np.array_equal(sqr.decode(vmin, vdiff, codes), xb)
    assert np.array_equal(ix.sq_codes(), codes)
    dis = sqr.sq_distances(metric, vmin, vdiff, codes, xq)
    assert np.array_equal(dis, np.rint(dis))  # exact values
    for k in (1, 10, 100, 2048):
        D, I = ix.search(xq, k)
        _same(D, I, *sqr.sq_select(dis, k, metric), f"lattice k={k}")
        if k > 1:
            assert (D[:, -1] == D[:, -2]).any()  # the boundary is tied for some query


# ------------------------------------------------------------------------------------------------ overflow, Python-written images
@pytest.mark.parametrize("wrapped", [False, True])
def test_values_improving_with_the_row_overflow_the_buckets_and_are_rescanned(wrapped, tmp_path):
    """2 R + 5 rows whose codes are written through a file so that the distances DEcrease with the row number"""
    mf = _mf()
    R = _index(2, "SQ8", L2, np.zeros(2), np.ones(2)).get_stat("sq_rows_per_workgroup")
    n = 2 * R + 5
    assert n <= 65536
    # s = (256, 1), a = 0: the code (c0, c1) decodes to the point (256 c0, c1)
    vmin, vdiff = np.array([-128.0, -0.5], dtype=np.float32), np.array([256.0 * 255.0, 255.0], dtype=np.float32)
    v = np.arange(n)[::-1]  # row p holds the point (256 (v // 256), v % 256), v = n - 1 - p: closer to the left with every row
    codes = np.stack([v // 256, v % 256], axis=1).astype(np.uint8)
    assert np.array_equal(sqr.decode(vmin, vdiff, codes), np.stack([256.0 * (v // 256), v % 256], axis=1).astype(np.float32))
    ids = (np.arange(n, dtype=np.int64) * 5 + 3) if wrapped else None
    path = str(tmp_path / "descending.index")
    sqr.write_sq(path, 2, L2, vmin, vdiff, codes, ids=ids)
    ix = mf.read_index(path)
    inner = ix.index if wrapped else ix
    assert inner.kind == mf.KIND_SQ and ix.ntotal == n and ix.is_trained
    assert np.array_equal(ix.sq_codes(), codes)
    xq = np.array([[-10, 0], [-2000, 0], [70000, 7], [-10, 300]], dtype=np.float32)  # (the third: worsening with the row)
    dis = sqr.sq_distances(L2, vmin, vdiff, codes, xq)
    for k in (1, 10, 1000):
        D, I = ix.search(xq, k)
        _same(D, I, *sqr.sq_select(dis, k, L2, labels=ids), f"descending values k={k}")
        assert I[0, 0] == (ids[n - 1] if wrapped else n - 1)
        assert ix.get_stat("sq_scan_rescans") > 0
        assert ix.get_stat("sq_scan_launches") > ix.get_stat("sq_scan_rescans")


# ------------------------------------------------------------------------------------------------ selectors
@pytest.mark.parametrize("metric", [L2, IP])
def test_selectors_bare_and_under_idmap(metric):
    rng = np.random.default_rng(60 + metric)
    d, n = 12, 3000
    xb = _rows(rng, n, d)
    xq = _rows(rng, 15, d)
    vmin, vdiff = sqr.train_range(xb)
    codes = sqr.encode(vmin, vdiff, xb)
    dis = sqr.sq_distances(metric, vmin, vdiff, codes, xq)
    ids = rng.permutation(3 * n)[:n].astype(np.int64)
    for how in ("bare", "IDMap"):
        ix = _index(d, "SQ8" if how == "bare" else "IDMap,SQ8", metric, vmin, vdiff)
        ix.add(xb) if how == "bare" else ix.add_with_ids(xb, ids)
        lab = np.arange(n, dtype=np.int64) if how == "bare" else ids
        _same(*ix.search(xq, 10), *sqr.sq_select(dis, 10, metric, labels=lab), how + ", no selector")
        for keep in (lab % 3 == 0, np.arange(n) >= 2900):
            for k in (10, 1500):
                Dr, Ir = sqr.sq_select(dis, k, metric, labels=lab, keep=keep)
                _same(*ix.search(xq, k, sel=("bitmap", bitmap_from_ids(lab, keep))), Dr, Ir, f"{how} bitmap k={k}")
                _same(*ix.search(xq, k, sel=("batch", lab[keep])), Dr, Ir, f"{how} batch k={k}")
        D, I = ix.search(xq, 10, sel=("batch", np.array([3 * n + 5], dtype=np.int64)))
        assert (I == -1).all() and (D == (sqr.FLT_MAX if metric == L2 else -sqr.FLT_MAX)).all()


# ------------------------------------------------------------------------------------------------ persistence, placement
@pytest.mark.parametrize("desc", ["SQ8", "IDMap,SQ8"])
def test_write_read_clone_and_refused_sharding(desc, tmp_path):
    mf = _mf()
    rng = np.random.default_rng(71)
    d, n = 21, 2500
    xb = _rows(rng, n, d)
    xq = _rows(rng, 10, d)
    vmin, vdiff = sqr.train_range(xb)
    wrapped = desc.startswith("IDMap")
    ids = rng.permutation(10 * n)[:n].astype(np.int64) if wrapped else None
    ix = _index(d, desc, IP, vmin, vdiff)
    ix.add(xb) if ids is None else ix.add_with_ids(xb, ids)
    codes = sqr.encode(vmin, vdiff, xb)
    Dr, Ir = sqr.sq_search(IP, vmin, vdiff, codes, xq, 20, labels=ids)
    _same(*ix.search(xq, 20), Dr, Ir, desc)
    # write -> the Python parser sees the model's codes; read_index gives equal codes and an equal search
    path = str(tmp_path / "a.index")
    mf.write_index(ix, path)
    img = sqr.parse_sq(path)
    assert (img["d"], img["ntotal"], img["trained"], img["metric"]) == (d, n, True, IP)
    assert (img["qtype"], img["rangestat"], img["rangestat_arg"], img["sq_code_size"]) == (0, 0, 0.0, d)
    assert np.array_equal(img["vmin"].view(np.uint32), vmin.view(np.uint32)) and np.array_equal(img["vdiff"].view(np.uint32), vdiff.view(np.uint32))
    assert np.array_equal(img["codes"], codes)
    assert (img["ids"] is None) if ids is None else np.array_equal(img["ids"], ids)
    back = mf.read_index(path)
    assert back.ntotal == n and back.is_trained and np.array_equal(back.sq_codes(), codes)
    _same(*back.search(xq, 20), Dr, Ir, desc + " after read_index")
    # a Python-written file loads and searches identically
    path2 = str(tmp_path / "b.index")
    sqr.write_sq(path2, d, IP, vmin, vdiff, codes, ids=ids)
    _same(*mf.read_index(path2).search(xq, 20), Dr, Ir, desc + " from a Python-written file")
    # another quantiser type is refused on reading
    path3 = str(tmp_path / "refused.index")
    sqr.write_sq(path3, d, IP, vmin, vdiff, codes, ids=ids, qtype=1)
    with pytest.raises(mf.FaissException, match="qtype = 1"):
        mf.read_index(path3)
    # clone_to_gpu(0): an independent copy; to_gpu(0) in place
    clone = ix.clone_to_gpu(0)
    ix.add(xq) if ids is None else ix.add_with_ids(xq, np.arange(10) + 10**6)
    assert clone.ntotal == n and ix.ntotal == n + 10
    _same(*clone.search(xq, 20), Dr, Ir, desc + " clone")
    clone.to_gpu(0)
    _same(*clone.search(xq, 20), Dr, Ir, desc + " clone after to_gpu")
    # sharding is refused and leaves the index as it was
    before = clone.search(xq, 5)
    with pytest.raises(mf.FaissException, match="This index type is not implemented"):
        clone.shard_to_gpus([0, 0])
    with pytest.raises(mf.FaissException, match="This index type is not implemented"):
        clone.clone_to_gpu(-1)
    if mf.device_count() >= 2:
        with pytest.raises(mf.FaissException, match="This index type is not implemented"):
            clone.shard_to_gpus([0, 1])
    assert clone.shard_info() is None and clone.ntotal == n
    _same(*clone.search(xq, 5), *before, desc + " after the refused sharding")
    # an untrained, empty index round-trips too
    path4 = str(tmp_path / "c.index")
    mf.write_index(mf.index_factory(d, desc, L2), path4)
    empty = mf.read_index(path4)
    assert not empty.is_trained and empty.ntotal == 0 and empty.d == d


def test_sharded_factory_is_refused():
    """env MVS_DEVICES at creation: a fresh process, as the variable is read when the index is made"""
    code = (
        "import sys; sys.path.insert(0, %r); import mi355_faiss as mf\n"
        "try:\n    mf.index_factory(8, 'IDMap,SQ8', 1)\nexcept mf.FaissException as e:\n    print('REFUSED', e)\n"
    ) % os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, MVS_DEVICES="0,0"))
    assert out.returncode == 0, out.stderr
    assert "REFUSED" in out.stdout and "This index type is not implemented" in out.stdout


# ------------------------------------------------------------------------------------------------ factory, errors
def test_factory_strings_and_refusals():
    mf = _mf()
    for desc in ("SQ8", "IDMap,SQ8", "IDMap2,SQ8"):
        ix = mf.index_factory(8, desc, IP)
        inner = ix.index if desc.startswith("IDMap") else ix
        assert inner.kind == mf.KIND_SQ and not ix.is_trained and inner.quantizer is None and ix.nlist == 0
    assert mf.index_factory(2048, "SQ8", L2).d == 2048
    for desc, dd in (("SQ4", 8), ("SQ6", 8), ("SQfp16", 8), ("SQ8_direct", 8), ("SQbf16", 8), ("SQ8", 2049), ("IDMap,SQ4", 8)):
        with pytest.raises(mf.FaissException, match="This index type is not implemented on the MI355X path yet: .*" + desc.split(",")[-1]):
            mf.index_factory(dd, desc, L2)
    with pytest.raises(mf.FaissException, match="metric type 2 is not implemented on the MI355X path"):
        mf.index_factory(8, "SQ8", 2)
    x = _rows(np.random.default_rng(3), 40, 8)
    ix = _index(8, "SQ8", L2, *sqr.train_range(x))
    ix.add(x)
    with pytest.raises(mf.FaissException, match="2048"):
        ix.search(x[:1], 2049)
    with pytest.raises(mf.FaissException, match="k > 0"):
        ix.search(x[:1], 0)
    with pytest.raises(mf.FaissException, match="not an IVFSQ index"):
        ix.ivfsq_list_size(0)
    with pytest.raises(mf.FaissException, match="not an SQ index"):
        mf.index_factory(8, "Flat", L2).sq_trained()


# ------------------------------------------------------------------------------------------------ the glue
def test_idmap_sq8_through_the_cpp_glue_path():
    """boundary_driver ingest: chunked AddFunction from two threads (buffered: the index needs training), AddFinaliseFunction (train + add)"""
    out = subprocess.run([DRIVER, "ingest", "3000", "8", "2", "IDMap,SQ8"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ingest\tOK ntotal=3000" in out.stdout


# ------------------------------------------------------------------------------------------------ one loose sanity case
def test_recall_against_flat_is_not_below_the_models():
    """20 000 clustered rows at d = 64: recall@10 of SQ8 against Flat, reported; the yardstick is the same recall computed from the CPU
    model (the results are compared bitwise elsewhere), not a fixed number"""
    mf = _mf()
    rng = np.random.default_rng(5)
    d, n, nq, k = 64, 20000, 50, 10
    centres = rng.standard_normal((100, d)).astype(np.float32) * 4
    xb = (centres[rng.integers(0, 100, n)] + rng.standard_normal((n, d))).astype(np.float32)
    xq = (centres[rng.integers(0, 100, nq)] + rng.standard_normal((nq, d))).astype(np.float32)
    _, It = orc.flat_search(L2, xb, xq, k)
    ix = mf.index_factory(d, "SQ8", L2)
    ix.train(xb)
    ix.add(xb)
    _, I = ix.search(xq, k)
    vmin, vdiff = sqr.train_range(xb)
    _, Im = sqr.sq_search(L2, vmin, vdiff, sqr.encode(vmin, vdiff, xb), xq, k)

    def recall(J):
        return sum(np.intersect1d(J[q], It[q]).size for q in range(nq)) / (nq * k)

    print(f"recall@10 of SQ8 against Flat: device {recall(I):.4f}, CPU model {recall(Im):.4f}")
    assert recall(I) >= recall(Im)
