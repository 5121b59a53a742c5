"""bfKnn over bf16 matrices (include/mi355_faiss.h "brute-force k-NN on caller-owned matrices", csrc/bf_knn.hip): bf16
vectors scanned in place, queries of the three types rounded to bf16.  The float64 reference and its helpers are tests/test_bfknn_gpu.py's."""
import numpy as np
import pytest
from test_bfknn_gpu import FMAX, IP, L2, dev as base_dev, exact_scores, mf, reference, same_bits, tolerance  # noqa: F401  (mf: the fixture)

pytestmark = pytest.mark.gpu


def bf16_round(x):
    """f32 -> the nearest bf16 value as f32: round to nearest even on the upper 16 bits, a NaN quieted"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = np.where((b & 0x7FFFFFFF) > 0x7F800000, (b >> 16) | 0x40, (b + 0x7FFF + ((b >> 16) & 1)) >> 16)
    return (r.astype(np.uint32) << 16).view(np.float32)


def dev(a, kind, row_major=True, shift=0):
    """f32 numpy [m, d] -> a device tensor of dtype `kind` ("bf16": the upper 16 bits of each value) in the given layout and base shift"""
    import torch

    if kind != "bf16":
        return base_dev(a.astype(np.float16 if kind == "f16" else np.float32), row_major, shift)
    bits = (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)
    return base_dev(bits, row_major, shift).view(torch.bfloat16)


# (d, n, nq, k, vectors row-major, queries row-major, query dtype, base shift).  d: one k-step and its edges (odd d is ROW_STAGED), 72 and
# 128 in registers, 160 and 512 with LDS queries; n: a tile +- 1, the generation boundaries, 2049 with k = 2048, n < k; column-major with
# n % 8 == 0 (COL_DIRECT) and not (COL_STAGED); a base shifted by 2 bytes takes d % 8 == 0 through the staged path
INT_CASES = [
    (1, 63, 1, 1, True, True, "bf16", 0), (31, 64, 15, 10, True, False, "f16", 0), (32, 65, 16, 10, True, True, "f32", 0),
    (33, 255, 17, 100, True, True, "bf16", 0), (100, 256, 33, 10, True, False, "f32", 0), (72, 65, 33, 10, True, True, "bf16", 0),
    (128, 257, 130, 100, True, True, "bf16", 0), (128, 1025, 17, 10, False, True, "f16", 0), (128, 2049, 17, 2048, True, False, "f32", 0),
    (160, 63, 1, 100, True, True, "f32", 0), (160, 1024, 33, 10, False, True, "bf16", 0), (512, 257, 16, 10, True, True, "bf16", 0),
    (512, 64, 130, 10, False, False, "f16", 0), (32, 1025, 130, 1, True, True, "bf16", 1), (33, 256, 15, 10, False, True, "f32", 0),
]  # fmt: skip


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,n,nq,k,vrow,qrow,qkind,shift", INT_CASES)
def test_exact_on_integer_data(mf, metric, d, n, nq, k, vrow, qrow, qkind, shift):
    rng = np.random.default_rng(1000 * d + n)
    xb, xq = rng.integers(-3, 4, (n, d)).astype(np.float32), rng.integers(-3, 4, (nq, d)).astype(np.float32)
    D, I = mf.bf_knn_torch(dev(xb, "bf16", vrow, shift), dev(xq, qkind, qrow), k, metric)
    Dr, Ir = reference(metric, exact_scores(metric, xb, xq), k)
    assert np.array_equal(I.cpu().numpy(), Ir), np.argwhere(I.cpu().numpy() != Ir)[:4]
    assert same_bits(D.cpu().numpy(), Dr)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,n,nq,k,vrow", [(33, 1000, 17, 10, False), (64, 3000, 33, 10, True)])
def test_random_data_within_the_derived_bound(mf, metric, d, n, nq, k, vrow):
    """tolerance: 2^-22 (d + 4) (|qb|^2 + |h_i|^2), products of two bf16 values being exact.  Worst error / tol seen on the device: 0.0171"""
    rng = np.random.default_rng(d)
    xb, xq = bf16_round(rng.standard_normal((n, d))), bf16_round(rng.standard_normal((nq, d)))
    D, I = (t.cpu().numpy() for t in mf.bf_knn_torch(dev(xb, "bf16", vrow), dev(xq, "bf16"), k, metric))
    score, tol = exact_scores(metric, xb, xq), tolerance(xb, xq)
    key = score if metric == L2 else -score
    order = np.argsort(key, axis=1, kind="stable")[:, : k + 1]
    sk, tk = np.take_along_axis(key, order, 1), np.take_along_axis(tol, order, 1)[:, :k]
    gap_after = sk[:, 1:] - sk[:, :-1]
    gap_before = np.concatenate([np.full((nq, 1), np.inf), gap_after[:, :-1]], axis=1)
    sure = (gap_after > 2 * tk) & (gap_before > 2 * tk)
    err = np.abs(D.astype(np.float64) - np.take_along_axis(score, I, 1)) / np.take_along_axis(tol, I, 1)
    print("share of slots with clear gaps: %.3f, worst error / tol: %.4f" % (sure.mean(), err.max()))
    assert sure.mean() >= 0.9 and np.array_equal(I[sure], order[:, :k][sure]) and (err <= 1).all()


@pytest.mark.parametrize("metric", [L2, IP])
def test_rounding_norms_and_all_pairs(mf, metric):
    import torch

    d, n, k, rng = 33, 200, 10, np.random.default_rng(7)
    xb = bf16_round(rng.standard_normal((n, d)))
    xq = rng.standard_normal((8, d)).astype(np.float32)  # f32 values, not bf16 ones: the pack kernel rounds every component
    xq[0, 0] = np.uint32(0x3FFFFFFF).view(np.float32)  # just below 2: rounds up across the binade
    xq[1, 0], xq[1, 1] = 1 + 2.0**-8, 1 + 3 * 2.0**-8  # exact ties: to the even neighbours 1 and 1 + 2^-6
    xq[2, 0], xq[3, 0], xq[4, 0] = 3.4e38, 1e-39, np.nan  # beyond the largest bf16: +inf; a bf16 subnormal; a NaN
    qb = bf16_round(xq)
    assert qb[0, 0] == 2 and qb[1, 0] == 1 and qb[1, 1] == 1 + 2.0**-6 and qb[2, 0] == np.inf and 0 < qb[3, 0] < 2.0**-126 and np.isnan(qb[4, 0])
    finite = [0, 1, 3, 5, 6, 7]
    score, tol = exact_scores(metric, xb, qb[finite]), tolerance(xb, qb[finite])
    for vrow in (True, False):  # f32 queries give the bits of the same queries rounded here and passed as bf16
        tb = dev(xb, "bf16", vrow)
        D, I = mf.bf_knn_torch(tb, dev(xq, "f32"), k, metric)
        Db, Ib = mf.bf_knn_torch(tb, dev(qb, "bf16"), k, metric)
        assert torch.equal(I, Ib) and same_bits(D.cpu().numpy(), Db.cpu().numpy())
        assert (I[4] == -1).all() and (D[4] == float(FMAX if metric == L2 else -FMAX)).all()  # a NaN score is admitted nowhere
        P = mf.pairwise_distances_torch(tb, dev(xq, "f32"), metric).cpu().numpy()
        assert same_bits(P, mf.pairwise_distances_torch(tb, dev(qb, "bf16"), metric).cpu().numpy())
        assert np.isnan(P[4]).all() and (np.abs(P[finite].astype(np.float64) - score) <= tol).all()
    # supplied norms are n_i verbatim: integer data, each true norm + 1 -> every L2 distance + 1 exactly, inner product untouched
    xi, qi = rng.integers(-3, 4, (n, d)).astype(np.float32), rng.integers(-3, 4, (8, d)).astype(np.float32)
    norms = torch.from_numpy((xi * xi).sum(1) + 1).to("cuda:0")
    exact = exact_scores(metric, xi, qi) + (1 if metric == L2 else 0)
    D, I = mf.bf_knn_torch(dev(xi, "bf16"), dev(qi, "bf16"), k, metric, norms=norms)
    assert np.array_equal(I.cpu().numpy(), reference(metric, exact, k)[1]) and same_bits(D.cpu().numpy(), reference(metric, exact, k)[0])
    assert same_bits(mf.pairwise_distances_torch(dev(xi, "bf16"), dev(qi, "bf16"), metric, norms=norms).cpu().numpy(), exact.astype(np.float32))


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("vkind", ["f16", "f32"])
def test_bf16_queries_over_the_other_vector_types(mf, metric, vkind):
    d, n, nq, k, rng = 33, 1025, 17, 10, np.random.default_rng(11)
    tb = dev(rng.standard_normal((n, d)), vkind)
    xq = bf16_round(rng.standard_normal((nq, d)))
    D, I = mf.bf_knn_torch(tb, dev(xq, "bf16"), k, metric)
    Dw, Iw = mf.bf_knn_torch(tb, dev(xq, "f32"), k, metric)  # the same queries widened exactly
    assert np.array_equal(I.cpu().numpy(), Iw.cpu().numpy()) and same_bits(D.cpu().numpy(), Dw.cpu().numpy())
