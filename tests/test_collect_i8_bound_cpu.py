"""The int8 store's coarse bound restated on the CPU (csrc/flat_collect.hip "int8 store"): rows Y = clamp(rint(y' / sy)),
queries Q = clamp(rint(a / sa)) with sa = alpha sy and unit = alpha sy^2 powers of two, beta_int = rint(beta / unit), s = unit (beta_int +
<Q, Y>) computed exactly in integers; E_i8 = ||a - sa Q|| max||y'|| + (||a|| + ||a - sa Q||) max||y' - sy Y|| + unit / 2 bounds
|s - (alpha <x', y'> + beta)|, and the integer pass bound ceil(p / unit) admits exactly the rows the real test s >= p admits."""

import math

import numpy as np
import pytest


def _q(v, inv_s):
    return np.clip(np.rint(v * inv_s), -128, 127).astype(np.int64)


def _setup(yc, alpha, amax=None):
    amax = float(np.abs(yc).max()) if amax is None else amax
    sy = 2.0 ** math.ceil(math.log2(amax / (128 * 1.01)))
    return sy, alpha * sy, alpha * sy * sy


def _check(yc, xc, alpha, sy=None):
    if sy is None:
        sy, sa, unit = _setup(yc, alpha)
    else:
        sa, unit = alpha * sy, alpha * sy * sy
    yc = yc.astype(np.float32)
    Y = _q(yc, np.float32(1.0 / sy))
    ry = yc.astype(np.float64) - sy * Y
    ndy = math.sqrt(float((ry * ry).sum(1).max()))
    ync = math.sqrt(float((yc.astype(np.float64) ** 2).sum(1).max()))
    beta = -(yc.astype(np.float64) ** 2).sum(1) if alpha == 2 else yc.astype(np.float64).sum(1) * 0.25
    bint = np.rint(beta / unit).astype(np.int64)
    sints = []
    for x in xc:
        a = (alpha * x).astype(np.float32)
        Q = _q(a, np.float32(1.0 / sa))
        rq = a.astype(np.float64) - sa * Q
        ndq = math.sqrt(float((rq * rq).sum()))
        na = math.sqrt(float((a.astype(np.float64) ** 2).sum()))
        E = ndq * ync + (na + ndq) * ndy + 0.5 * unit
        sint = bint + Y @ Q
        assert np.abs(sint).max() < 2**24
        s = sint.astype(np.float64) * unit
        exact = yc.astype(np.float64) @ a.astype(np.float64) + beta
        assert np.all(np.abs(s - exact) <= E * (1 + 1e-9)), float(np.abs(s - exact).max() / E)
        # the integer pass bound of a real one: never rejects what s >= p admits, never admits what it rejects
        for p in (float(np.quantile(s, 0.9)), float(s.max()), float(s.min()) - 1.0, float(np.float32(s[3] + unit * 0.25))):
            pf = np.float32(p)
            t = _thr_f32(pf, np.float32(1.0 / unit))  # (the kernel's f32 arithmetic)
            assert np.array_equal(sint >= t, s >= float(pf))
        sints.append(sint)
    return np.stack(sints), ndy


@pytest.mark.parametrize("alpha", [2, 1])
def test_i8_bound_holds_on_uniform_rows(alpha):
    rs = np.random.RandomState(alpha)
    y = rs.rand(4000, 128).astype(np.float32)
    mu = y.mean(0)
    _check(y - mu, rs.rand(20, 128).astype(np.float32) - mu, alpha)


@pytest.mark.parametrize("alpha", [2, 1])
def test_i8_bound_holds_on_adversarial_rows(alpha):
    rs = np.random.RandomState(10 + alpha)
    y = (rs.rand(2000, 128).astype(np.float32) - 0.5)
    sy = 2.0**-8
    y[0] = 128 * sy * 1.3  # every component clamped at +127 (and -128 below)
    y[1] = -128 * sy * 1.3
    y[2] = np.where(np.arange(128) % 2 == 0, 0.5, -0.5)  # the largest norm
    y[3] = y[4]  # ties
    y[5, :] = (np.arange(128) + 0.5) * sy  # halves: rint's ties to even
    x = rs.rand(10, 128).astype(np.float32) - 0.5
    x[0] = 4.0  # a query far outside the store's range: its clamp residual widens only its own E
    _check(y, x, alpha, sy=sy)


def _thr_f32(p, inv_unit):
    """cl_i8_thr (csrc/flat_collect.h) in float32, step for step: ceil(p * inv_unit), NaN and > 2^30 -> INT_MAX, < -2^30 -> -(2^31 - 1)"""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.ceil(np.float32(p) * np.float32(inv_unit))
    if np.isnan(t) or t > np.float32(1073741824.0):
        return 2**31 - 1
    if t < np.float32(-1073741824.0):
        return -(2**31 - 1)
    return int(t)


@pytest.mark.parametrize("k", [-15, -16, -9, 3])
def test_i8_integer_threshold_matches_the_real_test(k):
    """s_int >= cl_i8_thr(p) exactly when the f32 value s = s_int * unit passes s >= p -- for bounds on the grid, between grid points, a
    float32 ulp off it, subnormal, huge, infinite and NaN ones; and the outlier rows' beta_int = INT_MIN passes none of them"""
    unit = np.float32(2.0**k)
    inv = np.float32(1.0) / unit
    rs = np.random.RandomState(k + 40)
    sint = np.concatenate([rs.randint(-(2**24) + 1, 2**24, 4000), np.arange(-40, 41), [2**24 - 1, -(2**24) + 1]]).astype(np.int64)
    s = sint.astype(np.float32) * unit  # exact: |s_int| < 2^24, unit a power of two
    assert np.array_equal(s.astype(np.float64), sint.astype(np.float64) * float(unit))
    fmax = np.finfo(np.float32).max
    ps = [np.float32(v) for v in (0.0, -0.0, 1e-40, -1e-40, 1e30, -1e30, np.inf, -np.inf, np.nan, fmax, -fmax)]
    with np.errstate(over="ignore"):
        ps.append(np.float32(-fmax) - np.float32(3.5))  # B = -FLT_MAX (no bound yet) minus 2E: rounds to -FLT_MAX
        ps.append(np.float32(-fmax) - np.float32(1e38))  # ... or overflows to -inf
    for j in rs.randint(0, len(s), 60):
        v = s[j]
        ps += [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf)), v + unit * np.float32(0.5), v - unit * np.float32(0.25)]
    for p in ps:
        t = _thr_f32(p, inv)
        with np.errstate(invalid="ignore"):
            real = s >= np.float32(p)
        assert np.array_equal(sint >= t, real), (float(p), t)
        assert not (-(2**31) >= t), "an outlier row (beta_int = INT_MIN, zero row) must never pass"


# ---- the same bound on the inputs of tests/test_collect_i8_hostile_gpu.py: narrow rows, rows added later, skewed queries, lattices, clusters


def _uniform(seed, n, nq, d=128):
    rs = np.random.RandomState(seed)
    y = rs.rand(n, d).astype(np.float32)
    x = rs.rand(nq, d).astype(np.float32)
    mu = y.mean(0)
    return y - mu, x - mu


@pytest.mark.parametrize("alpha", [2, 1])
@pytest.mark.parametrize("d", [17, 33, 65, 100])
def test_i8_bound_holds_on_narrow_rows_padded_to_128(alpha, d):
    """d < 128: the store's rows and the query fragments are zero beyond d -- the padding adds nothing to <Q, Y> nor to a residual"""
    y, x = _uniform(200 + d + alpha, 3000, 12, d)
    yp, xp = np.zeros((len(y), 128), np.float32), np.zeros((len(x), 128), np.float32)
    yp[:, :d], xp[:, :d] = y, x
    s_pad, ndy_pad = _check(yp, xp, alpha)
    s_raw, ndy_raw = _check(y, x, alpha)
    assert np.array_equal(s_pad, s_raw) and ndy_pad == ndy_raw


@pytest.mark.parametrize("alpha", [2, 1])
def test_i8_bound_holds_on_rows_added_after_the_scales_were_fixed(alpha):
    """rows three times as far from the mean as the rows the scales were taken from: they clamp, the residual maximum grows, the bound holds"""
    y, x = _uniform(300 + alpha, 3000, 12)
    sy = _setup(y, alpha)[0]
    late = 3.0 * y[:64]
    assert np.abs(late).max() > 128 * sy * 1.5  # (they do clamp)
    _, ndy_first = _check(y, x, alpha, sy=sy)
    _, ndy_all = _check(np.concatenate([y, late]), x, alpha, sy=sy)
    assert ndy_all > 10 * ndy_first


@pytest.mark.parametrize("alpha", [2, 1])
@pytest.mark.parametrize("skew", ["x4", "+1"])
def test_i8_bound_holds_on_a_skewed_query_batch(alpha, skew):
    """every query of the batch outside the range sa was chosen for: scaled by four about the mean, or offset by one per component"""
    y, x = _uniform(400 + alpha, 3000, 12)
    x = 4.0 * x if skew == "x4" else x + np.float32(1.0)
    sy, sa, _ = _setup(y, alpha)
    assert (np.abs(alpha * x).max(1) > 128 * sa).all()  # (every query clamps)
    _check(y, x, alpha, sy=sy)


@pytest.mark.parametrize("alpha", [2, 1])
def test_i8_bound_holds_on_lattice_rows(alpha):
    """rows and queries on the half steps of sy: rint's ties to even decide most components"""
    rs = np.random.RandomState(500 + alpha)
    sy = 2.0**-8
    y = (rs.randint(-255, 256, (3000, 128)) * (sy / 2)).astype(np.float32)
    x = (rs.randint(-255, 256, (12, 128)) * (sy / 4)).astype(np.float32)
    assert (np.abs(y / sy - np.rint(y / sy)) == 0.5).mean() > 0.4
    _check(y, x, alpha, sy=sy)
    y1 = rs.randint(-1, 2, (3000, 128)).astype(np.float32)  # {-1, 0, 1}: equal s_int everywhere
    _check(y1, rs.randint(-1, 2, (12, 128)).astype(np.float32), alpha)


@pytest.mark.parametrize("alpha", [2, 1])
@pytest.mark.parametrize("d", [128, 48])
def test_i8_bound_holds_on_clustered_rows(alpha, d):
    from oracle import oracle as orc

    y = orc.synth_clustered(4000, d, 77, n_centers=256, sigma=0.05)
    x = y[::400] + np.float32(0.01)
    mu = y.mean(0)
    yp, xp = np.zeros((len(y), 128), np.float32), np.zeros((len(x), 128), np.float32)
    yp[:, :d], xp[:, :d] = y - mu, x - mu
    _check(yp, xp, alpha)


@pytest.mark.parametrize("metric", [1, 0])
def test_the_models_format_rule_on_four_fixtures(metric):
    """tests/i8_store_reference.py on data whose answer is known: uniform rows get the int8 store, one column of 4000 x the others' span
    and rows that are all equal (amax = 0) keep bf16, tight clusters whatever the rule's two error terms say -- none of them near a threshold"""
    import i8_store_reference as ref
    from oracle import oracle as orc

    rs = np.random.RandomState(600 + metric)
    n = 100_000  # (fewer rows: the mean's noise alone pushes max |y'| past 1.01 x 128 x 2^-8 and costs a bit of resolution)
    uni = rs.rand(n, 128).astype(np.float32)
    m = ref.StoreModel(uni, n, metric)
    assert m.decided() == "int8", m.describe()
    assert m.sy == 2.0**-8 and m.tau == math.inf and m.outlier_rows().size == 0
    assert abs(m.mu - 0.5).max() < 0.02
    spiky = uni.copy()
    spiky[:, 17] *= 4000.0
    m = ref.StoreModel(spiky, n, metric)
    assert m.decided() == "bf16" and m.ratio > 4.0 * ref.RATIO_BAND, m.describe()
    m = ref.StoreModel(np.tile(uni[:1], (n, 1)), n, metric)
    assert m.decided() == "bf16" and m.amax == 0.0
    clu = orc.synth_clustered(n, 48, 5, n_centers=256, sigma=0.05)
    m = ref.StoreModel(clu, n, metric)
    want = "int8" if m.ratio <= 4.0 and m.beta_max() < m.limit else "bf16"
    assert m.decided() == want and not 4.0 / ref.RATIO_BAND < m.ratio < 4.0 * ref.RATIO_BAND, m.describe()
    # the threshold exists from 262 144 rows on, and a row of 100 x the usual norm is beyond it
    big = rs.rand(ref.MIN_ROWS, 32).astype(np.float32)
    big[[5, 70000]] *= 100.0
    m = ref.StoreModel(big, len(big), metric)
    assert 64 * 32 / 12.0 * 0.9 < m.tau < 64 * 32 / 12.0 * 1.4 and list(m.outlier_rows()) == [5, 70000]
    assert m.decided() == "int8", m.describe()
    assert m.clamped_share(big[:100]) < 0.5 and m.clamped_share(4.0 * (big[:100] - 0.5) + 0.5) > 0.9
