"""Half-precision Flat (include/mi355_faiss.h "half-precision Flat", csrc/flat_f16.hip) through the C ABI: a Flat index
cloned with use_float16.  Integer data is compared bit for bit with a numpy int64 reference ordered by (score, row); random data within
the bound derived below; the store, the images, determinism, the admission rule and the refusals."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2, IP = 1, 0
FMAX = np.float32(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss as m

    assert m.device_count() >= 1
    return m


def clone16(mf, metric, xb, ids=None):
    src = mf.index_factory(xb.shape[1], "Flat" if ids is None else "IDMap,Flat", metric)
    if ids is None:
        src.add(xb)
    else:
        src.add_with_ids(xb, ids)
    ix = src.clone_to_gpu(0, use_float16=True)
    assert (ix.kind if ids is None else ix.index.kind) == mf.KIND_FLAT16 and ix.ntotal == len(xb) and ix.is_trained
    return ix


def reference(metric, score, k, allowed, labels):
    """score [nq][n] float64 (exact), the k best by (score, row) among the allowed rows -> D float32, I int64, padded"""
    nq, n = score.shape
    D = np.full((nq, k), FMAX if metric == L2 else -FMAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    rows = np.flatnonzero(allowed)
    for q in range(nq):
        s = score[q, rows]
        order = rows[np.lexsort((rows, s if metric == L2 else -s))][:k]
        D[q, : len(order)] = score[q, order]
        I[q, : len(order)] = labels[order]
    return D, I


def bitmap_of(ids, nbits):
    bits = np.zeros(nbits // 8 + 1, dtype=np.uint8)
    np.bitwise_or.at(bits, ids >> 3, (1 << (ids & 7)).astype(np.uint8))
    return bits


# (d, n, nq, k, idmap): every d where the row layout or the kernel changes (one k-step, its edges, 3 and 4 steps in registers, 5 and 16 from
# LDS), n at a row tile (64) +- 1, at the generation boundaries (256, 1024; 2048 rows first at k = 2048) +- 1 and below k, nq at a query
# group (16), at two, and beyond a wave's 64 queries and a workgroup's 32 (d > 128)
INT_CASES = [
    (1, 63, 1, 1, False), (31, 64, 15, 10, False), (32, 65, 17, 10, False), (33, 255, 33, 100, False), (100, 256, 17, 10, False),
    (128, 257, 33, 100, False), (128, 1025, 130, 10, False), (160, 1023, 33, 10, False), (512, 1024, 17, 100, False),
    (128, 2049, 15, 2048, False), (160, 50, 17, 100, False), (64, 7, 1, 10, False),
    (33, 1025, 17, 10, True), (128, 257, 33, 100, True), (160, 300, 15, 10, True),
]  # fmt: skip


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,n,nq,k,idmap", INT_CASES)
def test_exact_on_integer_data(mf, metric, d, n, nq, k, idmap):
    rng = np.random.default_rng(1000 * d + n)
    xb = rng.integers(-3, 4, (n, d)).astype(np.float32)
    xq = rng.integers(-3, 4, (nq, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64) * 7 + 3 if idmap else None
    labels = ids if idmap else np.arange(n, dtype=np.int64)
    ix = clone16(mf, metric, xb, ids)
    b64, q64 = xb.astype(np.int64), xq.astype(np.int64)
    ipm = q64 @ b64.T
    score = ((q64 * q64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :] - 2 * ipm if metric == L2 else ipm).astype(np.float64)
    some = labels[rng.random(n) < 0.5]
    if some.size == 0:
        some = labels[:1]
    lo, hi = int(np.percentile(labels, 20)), int(np.percentile(labels, 90))
    selectors = [
        (None, np.ones(n, dtype=bool)),
        (("bitmap", bitmap_of(some, int(labels.max()))), np.isin(labels, some)),
        (("batch", some), np.isin(labels, some)),
        (("and", ("range", lo, hi), ("not", ("batch", some))), (labels >= lo) & (labels < hi) & ~np.isin(labels, some)),
    ]
    for sel, allowed in selectors:
        D, I = ix.search(xq, k, sel=sel)
        Dr, Ir = reference(metric, score, k, allowed, labels)
        assert np.array_equal(I, Ir), (sel and sel[0], np.argwhere(I != Ir)[:4])
        assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32)), (sel and sel[0],)


# tol(q, i) = 2^-22 (d + 4) (|qh|^2 + |h_i|^2): products of two fp16 values are exact in f32; each 32-term instruction is charged 64 u of
# its largest partial sum (three times what the bf16 instruction is charged), ceil(d / 32) of them chained; the two norm chains gamma_d
# each; three final roundings (m_q + n_i, the fmaf, the clamp's operand).  |partial sums| <= (|qh|^2 + |h|^2) / 2 by Cauchy-Schwarz
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,n,nq,k", [(33, 1000, 17, 10), (64, 3000, 33, 10)])
def test_random_data_within_the_derived_bound(mf, metric, d, n, nq, k):
    rng = np.random.default_rng(d)
    xb = rng.standard_normal((n, d)).astype(np.float16).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float16).astype(np.float32)
    ix = clone16(mf, metric, xb)
    D, I = ix.search(xq, k)
    b64, q64 = xb.astype(np.float64), xq.astype(np.float64)
    qn, bn = (q64 * q64).sum(1), (b64 * b64).sum(1)
    ipm = q64 @ b64.T
    score = np.maximum(qn[:, None] + bn[None, :] - 2 * ipm, 0.0) if metric == L2 else ipm
    tol = 2.0**-22 * (d + 4) * (qn[:, None] + bn[None, :])
    key = score if metric == L2 else -score
    order = np.argsort(key, axis=1, kind="stable")[:, : k + 1]
    sk = np.take_along_axis(key, order, 1)
    tk = np.take_along_axis(tol, order, 1)
    gap_after = sk[:, 1:] - sk[:, :-1]  # [nq][k]: slot j to slot j + 1
    gap_before = np.concatenate([np.full((nq, 1), np.inf), gap_after[:, :-1]], axis=1)
    sure = (gap_after > 2 * tk[:, :k]) & (gap_before > 2 * tk[:, :k])
    print("share of slots with clear gaps: %.3f" % sure.mean())
    assert sure.mean() >= 0.9
    assert np.array_equal(I[sure], order[:, :k][sure])
    got_tol = np.take_along_axis(tol, I, 1)
    err = np.abs(D.astype(np.float64) - np.take_along_axis(score, I, 1))
    print("worst error / tol: %.4f" % (err / got_tol).max())
    assert (err <= got_tol).all()


def test_store_and_images(mf, tmp_path):
    from oracle import oracle as orc

    d, n = 33, 200
    rng = np.random.default_rng(7)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xb[3, 0], xb[4, 5], xb[5, 32] = 70000.0, -1e6, 65520.0  # overflow to +-inf (65520 is the first value that rounds up to it)
    xb[6, :4] = [6e-8, 3e-6, -2.5e-5, 5.9e-8]  # fp16 subnormals
    xb[7, 1] = 2.9e-8  # below half the smallest subnormal: +0
    with np.errstate(over="ignore"):
        dec = xb.astype(np.float16).astype(np.float32)
    src = mf.index_factory(d, "Flat", L2)
    src.add(xb)
    ix = src.clone_to_gpu(0, use_float16=True)
    assert ix.kind == mf.KIND_FLAT16 and src.clone_to_gpu(0).kind == mf.KIND_FLAT and ix.clone_to_gpu(0).kind == mf.KIND_FLAT
    assert np.array_equal(ix.reconstruct_n(0, n).view(np.uint32), dec.view(np.uint32))
    assert np.array_equal(ix.reconstruct(6).view(np.uint32), dec[6].view(np.uint32))
    assert 0 < ix.get_stat("flat16_device_bytes") <= (2 * 64 + 4) * (n + 63)
    # the image is a Flat image of the decoded rows: its exact search is the oracle's Flat search on them
    finite = np.isfinite(dec).all(1)
    ok = mf.index_factory(d, "Flat", L2)
    ok.add(xb[finite])
    path = os.path.join(tmp_path, "f16.index")
    mf.write_index(ok.clone_to_gpu(0, use_float16=True), path)
    back = mf.read_index(path)
    assert back.kind == mf.KIND_FLAT and back.ntotal == int(finite.sum())
    xq = rng.standard_normal((5, d)).astype(np.float32)
    D, I = back.search(xq, 10)
    Do, Io = orc.flat_search(L2, dec[finite], xq, 10)
    assert np.array_equal(I, Io) and np.array_equal(D.view(np.uint32), Do.view(np.uint32))
    # the flag has no effect on another kind
    ivf = mf.index_factory(d, "IVF8,Flat", L2)
    ivf.train(xb[finite])
    ivf.add(xb[finite])
    assert ivf.clone_to_gpu(0, use_float16=True).kind == mf.KIND_IVFFLAT


@pytest.mark.parametrize("metric", [L2, IP])
def test_determinism(mf, metric):
    d, n = 100, 3000
    rng = np.random.default_rng(11)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((33, d)).astype(np.float32)
    src = mf.index_factory(d, "Flat", metric)
    src.add(xb)
    ix = src.clone_to_gpu(0, use_float16=True)
    D1, I1 = ix.search(xq[32:], 10)
    D33, I33 = ix.search(xq, 10)
    assert np.array_equal(I1[0], I33[32]) and np.array_equal(D1.view(np.uint32)[0], D33.view(np.uint32)[32])
    far = 1e-3 * rng.standard_normal((5000, d)).astype(np.float32)  # near the origin: farther than the 10th neighbour, lower products
    if metric == L2:
        far += 100.0
    ix.add(far)
    D2, I2 = ix.search(xq, 10)
    assert ix.ntotal == n + 5000 and I2.max() < n
    assert np.array_equal(I2, I33) and np.array_equal(D2.view(np.uint32), D33.view(np.uint32))


def test_rule_and_refusals(mf):
    d, n = 32, 300
    rng = np.random.default_rng(13)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xb[10, 3] = np.nan
    xb[20, 0] = 1e6  # +inf in fp16: an L2 score of +inf; under inner product -inf against a query whose component 0 is negative
    xq = rng.standard_normal((4, d)).astype(np.float32)
    xq[:, 0] = -np.abs(xq[:, 0]) - 0.5
    for metric in (L2, IP):
        src = mf.index_factory(d, "Flat", metric)
        src.add(xb)
        ix = src.clone_to_gpu(0, use_float16=True)
        D, I = ix.search(xq, n)
        assert not np.isin(I, [10, 20]).any() and (I[:, : n - 2] >= 0).all() and (I[:, n - 2 :] == -1).all()
        assert np.isfinite(D[:, : n - 2]).all() and (D[:, n - 2 :] == (FMAX if metric == L2 else -FMAX)).all()
    text = "This index type is not implemented on the MI355X path yet"
    other = mf.index_factory(d, "Flat", L2).clone_to_gpu(0, use_float16=True)
    for call in (
        lambda: ix.range_search(xq, 1.0),
        lambda: ix.remove_ids(("batch", np.array([1], dtype=np.int64))),
        lambda: ix.merge_from(other),
        lambda: ix.search_and_reconstruct(xq, 3),
        lambda: ix.shard_to_gpus([0]),
        lambda: ix.clone_to_gpu(-1),
        lambda: src.clone_to_gpu(-1, use_float16=True),
        lambda: ix.search(xq, 2049),
        lambda: mf.index_factory(d, "Flat", 2).clone_to_gpu(0, use_float16=True),
        lambda: mf.index_factory(2049, "Flat", L2).clone_to_gpu(0, use_float16=True),
    ):
        with pytest.raises(Exception, match=text):
            call()
