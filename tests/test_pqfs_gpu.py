"""PQ<M>x4fs / IDMap,PQ<M>x4fs on the device against a numpy float32 model of the contract (include/mi355_faiss.h "4-bit product-quantised
indexes").  Rows, queries and codebooks are small integers: every T, lo and span is exact, the only roundings are the contract's single f32
operations, and labels and distance bits are compared for equality."""
import functools

import numpy as np
import pytest

from helpers import bitmap_from_ids
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
FLT_MAX = np.finfo(np.float32).max
NS, NQS, KS = (1, 17, 8192 + 33), (1, 17, 130), (1, 10, 2048)


def _mf():
    import mi355_faiss as mf

    return mf


def _data(M, dsub, n, seed=0):
    """codebooks with distinct values per (m, j) in every component, rows and queries: small integers"""
    rng = np.random.default_rng(1000 * M + 10 * dsub + seed)
    cb = np.stack([np.stack([rng.permutation(16) for _ in range(dsub)], axis=1) + m % 5 for m in range(M)]).astype(np.float32)
    xb = rng.integers(-4, 24, (n, M * dsub)).astype(np.float32)
    xq = rng.integers(-4, 24, (NQS[-1], M * dsub)).astype(np.float32)
    return cb, xb, xq


def _tables(cb, x, metric):
    """T[q][m][j], exact on integer input in any order of summation -> [nq, M, 16] f32"""
    M, _, dsub = cb.shape
    xs = x.reshape(x.shape[0], M, 1, dsub)
    return (((xs - cb[None]) ** 2) if metric == L2 else xs * cb[None]).sum(-1, dtype=np.float32)


def _encode(cb, x):
    return _tables(cb, x, L2).argmin(2).astype(np.uint8)  # (the first minimum: the smallest j)


def _pack(codes):
    return codes[:, 0::2] | (codes[:, 1::2] << 4)


@np.errstate(all="ignore")  # (a non-finite query's tables: the query is skipped below)
def _model(cb, codes, xq, k, metric, labels=None, keep=None):
    T = _tables(cb, xq, metric)
    lo, hi = T.min(2), T.max(2)
    span = (hi - lo).max(1)
    a = np.divide(np.float32(255), span, out=np.zeros_like(span), where=span != 0)
    b = functools.reduce(lambda s, m: s + lo[:, m], range(1, lo.shape[1]), lo[:, 0])
    # fmaf(T - lo, a, 0.5f): the product and the sum are exact in double, so one rounding to f32
    tq = np.floor(((T - lo[:, :, None]).astype(np.float64) * a[:, None, None] + 0.5).astype(np.float32)).clip(0, 255).astype(np.int64)
    s = sum(tq[:, m, :][:, codes[:, m]] for m in range(codes.shape[1]))  # [nq, n]
    rows = np.arange(codes.shape[0]) if keep is None else np.flatnonzero(keep)
    D = np.full((xq.shape[0], k), FLT_MAX if metric == L2 else -FLT_MAX, dtype=np.float32)
    I = np.full((xq.shape[0], k), -1, dtype=np.int64)
    for q in range(xq.shape[0]):
        if not np.isfinite(T[q]).all():
            continue
        sq = s[q, rows]
        order = np.lexsort((rows, sq if metric == L2 else -sq))[:k]
        D[q, : order.size] = b[q] + sq[order].astype(np.float32) / a[q] if a[q] != 0 else b[q]
        I[q, : order.size] = rows[order] if labels is None else labels[rows[order]]
    return D, I


def _same(got, ref, what):
    assert np.array_equal(got[1], ref[1]), f"{what}: labels differ in {(got[1] != ref[1]).sum()} slots"
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), f"{what}: distances differ in {(got[0] != ref[0]).sum()} slots"


def _index(desc, metric, cb, xb, ids=None):
    ix = _mf().index_factory(xb.shape[1], desc, metric)
    ix.pq_set_centroids(cb)
    ix.add(xb) if ids is None else ix.add_with_ids(xb, ids)
    return ix


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("dsub", [1, 3])
@pytest.mark.parametrize("M", [2, 6, 8, 34])
def test_search_equals_the_model(M, dsub, metric):
    for n in NS:
        cb, xb, xq = _data(M, dsub, n)
        codes = _encode(cb, xb)
        ix = _index(f"PQ{M}x4fs", metric, cb, xb)
        assert ix.kind == _mf().KIND_PQFS and ix.pq_info() == (M, 4)
        assert np.array_equal(ix.pq_codes(), _pack(codes)), f"n {n}: codes"
        ref = _model(cb, codes, xq, KS[-1], metric)  # once per n: a query's list is a prefix of its longest, alone or in a batch
        for nq in NQS:
            for k in KS:
                _same(ix.search(xq[:nq], k), (ref[0][:nq, :k], ref[1][:nq, :k]), f"n {n} nq {nq} k {k}")
        assert ix.last_kernel_info()["name"] == "pqfs_scan_kernel" and ix.get_stat("pqfs_scan_launches") == (2 if n > 8192 else 1)


@pytest.mark.parametrize("metric", [L2, IP])
def test_ties_come_back_in_row_order_and_a_query_alone_equals_itself_in_the_batch(metric):
    cb, xb, xq = _data(8, 3, 5)
    xb = np.tile(xb, (1700, 1))  # 8500 rows, every one 1700 times: two ranges full of ties
    ix = _index("PQ8x4fs", metric, cb, xb)
    D, I = ix.search(xq, 10)
    _same((D, I), _model(cb, _encode(cb, xb), xq, 10, metric), "duplicated rows")
    assert (np.diff(I, axis=1)[np.diff(D, axis=1) == 0] > 0).all()
    for q in (0, 16, 129):
        _same(ix.search(xq[q : q + 1], 10), (D[q : q + 1], I[q : q + 1]), f"query {q} alone")


@pytest.mark.parametrize("metric", [L2, IP])
def test_idmap_labels_bitmap_selector_zero_span_and_non_finite_queries(metric):
    cb, xb, xq = _data(6, 3, 300)
    codes = _encode(cb, xb)
    ids = np.arange(300, dtype=np.int64)[::-1] * 7 + 3
    ix = _index("IDMap,PQ6x4fs", metric, cb, xb, ids)
    xq = xq[:17].copy()
    xq[3, 4] = np.inf  # a non-finite table: only missing slots
    _same(ix.search(xq, 10), _model(cb, codes, xq, 10, metric, labels=ids), "IDMap")
    keep = np.arange(300) % 3 != 1
    _same(ix.search(xq, 10, sel=("bitmap", bitmap_from_ids(ids, keep))), _model(cb, codes, xq, 10, metric, labels=ids, keep=keep), "bitmap")
    flat = np.repeat(cb[:, :1], 16, axis=1)  # all-equal codebooks: span == 0, every score 0, the distance is b
    iz = _index("PQ6x4fs", metric, flat, xb)
    got = iz.search(xq[:3], 5)
    _same(got, _model(flat, _encode(flat, xb), xq[:3], 5, metric), "span == 0")
    assert np.array_equal(got[1], np.tile(np.arange(5), (3, 1)))


@pytest.mark.parametrize("d,M", [(8, 2), (18, 6)])
def test_train_add_and_reconstruct(d, M):
    mf = _mf()
    rng = np.random.default_rng(d)
    x = rng.standard_normal((500, d)).astype(np.float32)
    dsub = d // M
    ix = mf.index_factory(d, f"PQ{M}x4fs", L2)
    with pytest.raises(mf.FaissException, match="at least as large as number of clusters"):
        ix.train(x[:15])
    with pytest.raises(mf.FaissException, match="is_trained"):
        ix.add(x[:4])
    ix.train(x)
    cb = ix.pq_centroids()
    for m in range(M):
        o = orc.Index(dsub, "IVF16,Flat", orc.METRIC_L2)
        o.train(np.ascontiguousarray(x[:, m * dsub : (m + 1) * dsub]))
        assert np.array_equal(cb[m].view(np.uint32), o.ivf_centroids().view(np.uint32)), f"codebook {m}"
    cbi, xb, _ = _data(M, dsub, 100)
    ix = _index(f"PQ{M}x4fs", L2, cbi, xb)
    codes = _encode(cbi, xb)
    assert np.array_equal(ix.pq_codes(), _pack(codes)) and np.array_equal(ix.pq_codes(33, 20), _pack(codes)[33:53])
    rec = cbi[np.arange(M)[None, :], codes].reshape(100, d)
    assert np.array_equal(ix.reconstruct_n(0, 100), rec) and np.array_equal(ix.reconstruct(99), rec[99])
    assert np.array_equal(ix.reconstruct_batch([5, 98, 5]), rec[[5, 98, 5]])
    clone = ix.clone_to_gpu(0)  # through FAISS's packing and back into the tiled store
    assert clone.kind == mf.KIND_PQFS and np.array_equal(clone.pq_codes(), _pack(codes)) and np.array_equal(clone.pq_centroids(), cbi)
    with pytest.raises(mf.FaissException, match="add_with_ids not implemented"):
        ix.add_with_ids(xb[:2], np.arange(2))


def test_refusals(tmp_path):
    mf = _mf()
    for desc in ("PQ7x4fs", "PQ130x4fs", "IVF8,PQ4x4fs", "PQ4x4fs,RFlat", "PQ4x5fs"):
        with pytest.raises(mf.FaissException, match="This index type is not implemented on the MI355X path yet: "):
            mf.index_factory(7 * 130 * 4, desc, L2)
    cb, xb, xq = _data(4, 1, 20)
    ix = _index("IDMap,PQ4x4fs", L2, cb, xb, np.arange(20))
    for call in (lambda: mf.write_index(ix, str(tmp_path / "x.index")), lambda: ix.range_search(xq[:2], 5.0),
                 lambda: ix.remove_ids(("batch", np.arange(3)))):
        with pytest.raises(mf.FaissException, match="This index type is not implemented on the MI355X path yet: "):
            call()
    assert ix.ntotal == 20
