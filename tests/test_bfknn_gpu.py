"""bfKnn (include/mi355_faiss.h "brute-force k-NN on caller-owned matrices", csrc/bf_knn.hip) through bf_knn_torch: fp16
matrices scanned where they lie, row- and column-major, aligned and not.  Integer data is compared bit for bit with an int64 numpy
reference ordered by (score, row); random data with a half-precision Flat clone of the same rows (same bits) and with float64 inside the
bound tests/test_flat16_gpu.py derives for this arithmetic; then the options, the f32 route and the refusals."""
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


def dev(a, row_major=True, shift=0):
    """numpy [m, d] -> a device tensor of that shape and dtype, dense in the given layout, its base `shift` elements off an aligned one"""
    import torch

    src = np.ascontiguousarray(a if row_major else a.T)
    flat = torch.empty(src.size + shift, dtype=torch.from_numpy(src[:0]).dtype, device="cuda:0")
    flat[shift:] = torch.from_numpy(src.ravel()).to("cuda:0")
    t = flat[shift:].view(src.shape)
    return t if row_major else t.t()


def exact_scores(metric, xb, xq, norms=None):
    b, q = xb.astype(np.float64), xq.astype(np.float64)
    ip = q @ b.T
    if metric == IP:
        return ip
    return np.maximum((q * q).sum(1)[:, None] + ((b * b).sum(1) if norms is None else norms.astype(np.float64))[None, :] - 2 * ip, 0.0)


def reference(metric, score, k):
    """the k best of score [nq][n] by (score, row) -> D float32, I int64, padded with +-FLT_MAX / -1"""
    nq, n = score.shape
    D = np.full((nq, k), FMAX if metric == L2 else -FMAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    rows = np.arange(n)
    for q in range(nq):
        order = np.lexsort((rows, score[q] if metric == L2 else -score[q]))[:k]
        D[q, : len(order)] = score[q, order]
        I[q, : len(order)] = order
    return D, I


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# (d, n, nq, k, query dtype, queries row-major, base shift): d with unaligned rows (1, 7, 33), an aligned partial k-step (8, 40), the
# register / LDS boundary (128) and above it (160); n at a tile +- 1, with 65, 257, 1025 unaligned as columns; a shifted base takes an
# aligned shape through the staged path
INT_CASES = [
    (1, 63, 1, 1, np.float32, True, 0), (7, 64, 17, 10, np.float16, True, 0), (8, 65, 33, 10, np.float32, False, 0),
    (33, 257, 17, 100, np.float16, False, 0), (40, 1025, 130, 10, np.float32, True, 0), (128, 64, 33, 10, np.float16, True, 0),
    (128, 257, 130, 100, np.float32, False, 0), (128, 1025, 17, 10, np.float16, False, 0), (160, 63, 1, 10, np.float32, True, 0),
    (160, 1025, 33, 100, np.float16, True, 0), (33, 1025, 130, 1, np.float32, True, 0), (7, 257, 33, 100, np.float16, False, 0),
    (128, 2049, 17, 2048, np.float32, True, 0), (40, 64, 17, 10, np.float32, True, 1), (128, 1024, 33, 10, np.float16, True, 3),
    (160, 64, 17, 100, np.float32, False, 0),
]  # fmt: skip


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("vrow", [True, False])
@pytest.mark.parametrize("d,n,nq,k,qtype,qrow,shift", INT_CASES)
def test_exact_on_integer_data(mf, metric, vrow, d, n, nq, k, qtype, qrow, shift):
    rng = np.random.default_rng(1000 * d + n)
    xb = rng.integers(-3, 4, (n, d)).astype(np.float16)
    xq = rng.integers(-3, 4, (nq, d)).astype(qtype)
    D, I = mf.bf_knn_torch(dev(xb, vrow, shift), dev(xq, qrow), k, metric)
    Dr, Ir = reference(metric, exact_scores(metric, xb, xq), k)
    assert np.array_equal(I.cpu().numpy(), Ir), np.argwhere(I.cpu().numpy() != Ir)[:4]
    assert same_bits(D.cpu().numpy(), Dr)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("vrow", [True, False])
@pytest.mark.parametrize("d", [33, 128, 160])
def test_same_bits_as_half_precision_flat(mf, metric, vrow, d):
    rng = np.random.default_rng(d)
    xb = rng.standard_normal((1500, d)).astype(np.float32)
    xq = rng.standard_normal((33, d)).astype(np.float32)
    src = mf.index_factory(d, "Flat", metric)
    src.add(xb)
    Df, If = src.clone_to_gpu(0, use_float16=True).search(xq, 10)
    D, I = mf.bf_knn_torch(dev(xb.astype(np.float16), vrow), dev(xq), 10, metric)
    assert np.array_equal(I.cpu().numpy(), If) and same_bits(D.cpu().numpy(), Df)


def tolerance(xb, xq):  # 2^-22 (d + 4) (|q_h|^2 + |h_i|^2), as derived in tests/test_flat16_gpu.py
    b, q = xb.astype(np.float64), xq.astype(np.float64)
    return 2.0**-22 * (xb.shape[1] + 4) * ((q * q).sum(1)[:, None] + (b * b).sum(1)[None, :])


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,n,nq,k,vrow", [(33, 1000, 17, 10, False), (64, 3000, 33, 10, True)])
def test_random_data_within_the_derived_bound(mf, metric, d, n, nq, k, vrow):
    rng = np.random.default_rng(d)
    xb = rng.standard_normal((n, d)).astype(np.float16)
    xq = rng.standard_normal((nq, d)).astype(np.float16)
    D, I = (t.cpu().numpy() for t in mf.bf_knn_torch(dev(xb, vrow), dev(xq), k, metric))
    score, tol = exact_scores(metric, xb, xq), tolerance(xb, xq)
    key = score if metric == L2 else -score
    order = np.argsort(key, axis=1, kind="stable")[:, : k + 1]
    sk, tk = np.take_along_axis(key, order, 1), np.take_along_axis(tol, order, 1)
    gap_after = sk[:, 1:] - sk[:, :-1]
    gap_before = np.concatenate([np.full((nq, 1), np.inf), gap_after[:, :-1]], axis=1)
    sure = (gap_after > 2 * tk[:, :k]) & (gap_before > 2 * tk[:, :k])
    err = np.abs(D.astype(np.float64) - np.take_along_axis(score, I, 1))
    print("share of slots with clear gaps: %.3f, worst error / tol: %.4f" % (sure.mean(), (err / np.take_along_axis(tol, I, 1)).max()))
    assert sure.mean() >= 0.9
    assert np.array_equal(I[sure], order[:, :k][sure])
    assert (err <= np.take_along_axis(tol, I, 1)).all()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("option", ["all_random", "all_integer", "norms", "int32", "ignore"])
def test_options(mf, metric, option):
    import torch

    d, n, nq, k = 40, 257, 33, 10
    rng = np.random.default_rng(5)
    if option == "all_random":
        xb, xq = rng.standard_normal((n, d)).astype(np.float16), rng.standard_normal((nq, d)).astype(np.float16)
    else:
        xb, xq = rng.integers(-3, 4, (n, d)).astype(np.float16), rng.integers(-3, 4, (nq, d)).astype(np.float16)
    score = exact_scores(metric, xb, xq)
    for vrow in (True, False):
        tb, tq = dev(xb, vrow), dev(xq)
        if option.startswith("all"):  # k = -1: every score, no rule, no labels
            P = mf.pairwise_distances_torch(tb, tq, metric).cpu().numpy()
            assert P.shape == (nq, n)
            if option == "all_integer":
                assert same_bits(P, score.astype(np.float32))
            else:
                assert (np.abs(P.astype(np.float64) - score) <= tolerance(xb, xq)).all()
        elif option == "norms":  # deliberately not the true norms: used verbatim under L2, ignored under inner product
            fake = (np.arange(n) % 5 * 100).astype(np.float32)
            D, I = mf.bf_knn_torch(tb, tq, k, metric, norms=torch.from_numpy(fake).to("cuda:0"))
            Dr, Ir = reference(metric, exact_scores(metric, xb, xq, norms=fake), k)
            assert np.array_equal(I.cpu().numpy(), Ir) and same_bits(D.cpu().numpy(), Dr)
        elif option == "int32":
            D, I = mf.bf_knn_torch(tb, tq, k, metric)
            I32 = torch.full((nq, k), -7, dtype=torch.int32, device="cuda:0")
            D32, _ = mf.bf_knn_torch(tb, tq, k, metric, I=I32)
            assert np.array_equal(I32.cpu().numpy().astype(np.int64), I.cpu().numpy()) and same_bits(D32.cpu().numpy(), D.cpu().numpy())
        else:
            D = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda:0")
            _, I = mf.bf_knn_torch(tb, tq, k, metric, D=D, ignore_distances=True)
            assert (D == -7.0).all() and np.array_equal(I.cpu().numpy(), reference(metric, score, k)[1])


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("vrow,qtype", [(True, np.float16), (False, np.float32)])
def test_f32_vectors_equal_a_flat_index(mf, metric, vrow, qtype):
    d, n, nq, k = 33, 1025, 17, 10
    rng = np.random.default_rng(9)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(qtype)
    ix = mf.index_factory(d, "Flat", metric)
    ix.add(xb)
    Df, If = ix.search(xq.astype(np.float32), k)
    D, I = mf.bf_knn_torch(dev(xb, vrow), dev(xq, not vrow), k, metric)
    assert np.array_equal(I.cpu().numpy(), If) and same_bits(D.cpu().numpy(), Df)


@pytest.mark.parametrize("case", ["metric", "d", "k_large", "k_zero", "not_dense", "all_f32"])
def test_refusals(mf, case):
    import torch

    d = 2049 if case == "d" else 16
    xb = torch.zeros((2100, d), dtype=torch.float32 if case == "all_f32" else torch.float16, device="cuda:0")
    xq = torch.zeros((3, d), dtype=torch.float16, device="cuda:0")
    if case == "not_dense":
        with pytest.raises(ValueError, match="not dense"):
            mf.bf_knn_torch(xb[:, ::2], xq[:, ::2], 5, L2)
        return
    metric = 2 if case == "metric" else L2
    k = {"k_large": 2049, "k_zero": 0, "all_f32": -1}.get(case, 5)
    text = "'k > 0' failed" if case == "k_zero" else "not implemented on the MI355X path yet: bfKnn"
    with pytest.raises(mf.FaissException, match=text):
        mf.bf_knn_torch(xb, xq, k, metric)
