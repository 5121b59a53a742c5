"""The int8 store of the d <= 128 coarse filter (csrc/flat_coarse.hip ensure_h1_rows / ensure_i8_rows, csrc/flat_collect.hip "int8 store",
DESIGN.md 3.1) away from uniform d = 128 rows: narrow rows (17 <= d < 128, every row pitch of the f32 store), skewed rows, skewed query
batches, and rows added after the scales were fixed.  Every case returns the labels and the distance bits of the exact f32 kernel
(prefilter 0) on a fresh index of the same rows, and for the first 16 queries those of the CPU oracle; every case asserts the store the
model of tests/i8_store_reference.py predicts (get_stat "cl_store_i8") and the kernel that served it, so that none passes on another path.

The model's sums are float64 and the device's float32: each case first asserts, on the CPU, that its data is nowhere near a threshold
(test_case_data_is_not_borderline runs without a GPU).  The shadow clustering (option flat_shadow), which takes over L2 searches of
data that admits thousands of candidates per query, is off: these cases are about the stores behind flat_bf16_collect_kernel.
FlatIndex::reset() has no entry of its own in the C interface; case (p) empties the index through remove_ids, which drops every derived
store the same way (csrc/index.hip)."""

import functools

import numpy as np
import pytest

import i8_store_reference as ref

L2, IP = 1, 0
KERNEL = "flat_bf16_collect_kernel"
BASE = 262_144  # the smallest Flat index the int8 store serves
NQ = 300
TAIL = 77  # rows behind BASE: the last staged block and the last tile end inside
NARROW = [17, 32, 33, 64, 65, 100, 127]  # dp = 32 | 32, 64 | 64, 128 | 128 | 128: both sides of every pitch step, the smallest d, an odd one


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss

    return mi355_faiss


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    return oracle


# ---- data: built once per module, the same arrays for the CPU precondition and the GPU cases; never modified ---------------------------


def _rand(seed, n, d):
    return np.random.default_rng(seed).random((n, d), dtype=np.float32)


def _on_rows(xb, xq, rows):
    xq = xq.copy()
    xq[: len(rows)] = xb[rows]
    return xq


def _spread(lo, hi, cnt=16):
    return np.unique(np.linspace(lo, hi, cnt).astype(np.int64))


def _about_mean(rows, mu, f):
    return (mu + f * (rows - mu)).astype(np.float32)


def _uniform(d, seed):
    xb = _rand(seed, BASE + TAIL, d)
    return dict(xb=xb, xq=_on_rows(xb, _rand(seed + 1, NQ, d), _spread(0, len(xb) - 1)), on_rows=_spread(0, len(xb) - 1))


def _clustered(d):
    from oracle import oracle

    xb = oracle.synth_clustered(BASE + TAIL, d, 11 + d, n_centers=256, sigma=0.05)
    near = _spread(0, len(xb) - 1, NQ)
    return dict(xb=xb, xq=xb[near] + np.float32(0.01) * (_rand(12, len(near), d) - np.float32(0.5)))


def _offset(d):
    return dict(xb=_rand(21 + d, BASE + TAIL, d) + np.float32(100.0), xq=_rand(22, NQ, d) + np.float32(100.0))


def _colscale(d):
    sc = (30.0 ** (np.arange(d) / (d - 1.0))).astype(np.float32)  # 1 ... 30, geometrically
    # (d = 48 sits at a ratio of 3.8 ... 3.96 whatever the seed; this one is clear of the model's 3 % band)
    return dict(xb=_rand(84 + d, BASE + TAIL, d) * sc, xq=_rand(32, NQ, d) * sc)


def _lattice(d):
    rs = np.random.default_rng(41 + d)
    n = BASE + TAIL
    xb = rs.integers(-1, 2, (n, d), dtype=np.int8).astype(np.float32)
    dst, src = rs.choice(n, n // 10, replace=False), rs.choice(n, n // 10)
    xb[dst] = xb[src]  # about a tenth of the rows are copies of other rows
    xq = rs.integers(-1, 2, (NQ, d), dtype=np.int8).astype(np.float32)
    return dict(xb=xb, xq=_on_rows(xb, xq, np.concatenate([dst[:8], _spread(0, n - 1, 8)])))


def _sparse(d):
    rs = np.random.default_rng(51 + d)

    def draw(n):  # (the components that are not zero: uniform in [-1, 1))
        return (2 * rs.random((n, d), dtype=np.float32) - 1) * (rs.random((n, d), dtype=np.float32) < 0.1)

    xb, xq = draw(BASE + TAIL), draw(NQ)
    return dict(xb=xb, xq=_on_rows(xb, xq, _spread(0, len(xb) - 1)))


def _identical(d):
    return dict(xb=np.tile(_rand(61 + d, 1, d), (BASE + TAIL, 1)), xq=_rand(62, NQ, d))


def _spiky(d):
    xb, xq = _rand(71 + d, BASE + TAIL, d), _rand(72, NQ, d)
    xb[:, 17] *= 4000.0  # one column spans 4000 x the others: the int8 grid of the store would drown them
    xq[:, 17] *= 4000.0
    return dict(xb=xb, xq=xq)


def _skewed_queries():
    dat = _uniform(128, 81)
    xb, xq = dat["xb"], _rand(83, NQ, 128)
    mu = xb.mean(0)
    bad = xq.copy()
    for j, v in enumerate([np.nan, np.inf, -np.inf, 1e30, -1e30, np.nan, np.inf, -np.inf, 1e30, np.nan]):
        bad[NQ - 10 + j, (13 * j) % 128] = v
    return dict(xb=xb, xq=xq, x4=_about_mean(xq, mu, 4.0), plus1=xq + np.float32(1.0), bad=bad)


def _grown(later, n_first=BASE, seed=91):
    """uniform d = 128 rows; later(first rows, their mean, rs) -> the rows added after the first int8 search, in stages"""
    rs = np.random.default_rng(seed)
    first = rs.random((n_first, 128), dtype=np.float32)
    stages = [np.ascontiguousarray(s, dtype=np.float32) for s in later(first, first.mean(0), rs)]
    return dict(xb=np.concatenate([first] + stages), xq=rs.random((NQ, 128), dtype=np.float32), n_first=n_first,
                stages=list(np.cumsum([n_first] + [len(s) for s in stages])))  # fmt: skip


def _capacity(adds, dp=128):
    """FlatIndex::grow (csrc/index.hip): the row capacity after add() calls of these sizes -- the derived stores are allocated for it"""
    cap = n = 0
    for a in adds:
        n += a
        if n > cap:
            cap = max(n, (4 if cap * dp * 4 < (2 << 30) else 2) * cap + 4096)
    return cap


CHUNK = 1 << 16
CAP_AT_BASE = _capacity([CHUNK] * (BASE // CHUNK))  # 266 240: BASE rows added in 65 536-row calls
GROW_K = [1, 127, 129, CAP_AT_BASE + 1 - (BASE + 257)]  # ... the last one is the smallest count that crosses it


def _grow_k(first, mu, rs):
    return [rs.random((c, 128), dtype=np.float32) for c in GROW_K]


def _grow_clamp(first, mu, rs):  # (l), (q)
    return [_about_mean(first[1000:1064], mu, 3.0)]


def _grow_range_l2(first, mu, rs):  # (m) L2: beta_int = ||y'||^2 / unit ~ 36 x 10.7 x 2^15 = 1.3e7 > 2^23 - 2^21, ||y'||^2 ~ 385 < tau ~ 683
    return [_about_mean(first[1000:1064], mu, 6.0)]


def _grow_range_ip(first, mu, rs):
    # (m) inner product: beta = <mu, y>, unit = 2^-16, so the limit is beta ~ 96.  Scaling about the mean moves beta by f <mu, y - mu> ~ 1.6 f
    # only, and passes tau (f^2 x 10.7 > 683 at f = 8) long before: the rows move ALONG mu instead, by 15 -- beta ~ 32 + 15 ||mu|| ~ 117,
    # ||y'||^2 ~ 10.7 + 225 < tau
    return [(first[1000:1064] + 15.0 * mu / np.linalg.norm(mu)).astype(np.float32)]


def _grow_outliers(first, mu, rs):  # (n)
    return [first[[10, 20000, 200000]] * np.float32(100.0)]


def _grow_early(first, mu, rs):  # (o): searched at 70 000 rows, then grown to BASE + 1000 with two rows of 100 x the usual norm
    rest = rs.random((BASE + 1000 - len(first), 128), dtype=np.float32)
    rest[[150_000, len(rest) - 5]] *= 100.0
    return [rest]


DATA = {"uniform:48": lambda: _uniform(48, 5), "skewq": _skewed_queries, "k": lambda: _grown(_grow_k), "l": lambda: _grown(_grow_clamp),
        "m:1": lambda: _grown(_grow_range_l2), "m:0": lambda: _grown(_grow_range_ip), "n": lambda: _grown(_grow_outliers),
        "o": lambda: _grown(_grow_early, n_first=70_000), "spiky:48": lambda: _spiky(48)}  # fmt: skip
for _d in NARROW:
    DATA["narrow:%d" % _d] = functools.partial(_uniform, _d, 1000 + _d)
for _d in (128, 48):
    for _name, _fn in (("clustered", _clustered), ("offset", _offset), ("colscale", _colscale), ("lattice", _lattice), ("sparse", _sparse),
                       ("identical", _identical)):  # fmt: skip
        DATA["%s:%d" % (_name, _d)] = functools.partial(_fn, _d)


@functools.lru_cache(maxsize=3)
def _data(key):
    dat = DATA[key]()
    for v in dat.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return dat


@functools.lru_cache(maxsize=3)
def _model_l2(key):
    dat = _data(key)
    stages = dat.get("stages", [len(dat["xb"])])
    return ref.StoreModel(dat["xb"], dat.get("n_first", stages[0]), L2, n_i8=stages[0] if stages[0] >= BASE else stages[1])


def _model(key, metric):
    """the model of a case's rows, asserted to be away from every threshold at every row count the case searches at"""
    m = _model_l2(key).with_metric(metric)
    dat = _data(key)
    for n in dat.get("stages", [len(dat["xb"])]):
        if n >= m.n_i8:
            assert m.decided(n) != "borderline", "%s at %d rows is too near a threshold to test: %s" % (key, n, m.describe(n))
    return m


def test_case_data_is_not_borderline():
    """the precondition of every GPU case below, and what the model says of each (no GPU needed)"""
    verdicts = {L2: {}, IP: {}}
    for key in sorted(DATA):
        for metric in (L2, IP):
            m = _model(key, metric)
            dat = _data(key)
            verdicts[metric][key] = [m.decided(n) for n in dat.get("stages", [len(dat["xb"])]) if n >= m.n_i8]
    for metric in (L2, IP):
        _check_verdicts(verdicts[metric], metric)


def _check_verdicts(said, metric):
    assert said["narrow:17"] == ["int8"] and said["narrow:127"] == ["int8"] and said["uniform:48"] == ["int8"]
    assert said["spiky:48"] == ["bf16"] and said["identical:128"] == ["bf16"] and said["identical:48"] == ["bf16"]
    # (column scales 1 ... 30: most columns on a handful of levels -- still int8 at d = 48, ratio 3.8; declined at d = 128, ratio 4.5)
    assert said["colscale:128"] == ["bf16"] and said["colscale:48"] == ["int8"]
    assert said["offset:128"] == (["int8"] if metric == L2 else ["bf16"])  # (the centring absorbs the offset; <mu, y> / unit is past 2^24)
    assert said["k"] == ["int8"] * 5 and said["l"] == ["int8", "int8"] and said["n"] == ["int8", "int8"]
    assert said["m:%d" % metric] == ["int8", "bf16"]  # (the added rows break the range, below the outlier threshold)
    m = _model("m:%d" % metric, metric)
    assert m.outlier_rows().size == 0 and m.beta_max(BASE) < 0.9 * m.limit and m.beta_max() > 1.1 * m.limit
    assert list(_model("n", metric).outlier_rows()) == [BASE, BASE + 1, BASE + 2]
    m = _model("l", metric)
    assert m.residual_max() > 100 * m.residual_max(BASE)  # (the added rows clamp)
    assert _model("o", metric).tau == np.inf
    dat = _data("skewq")
    m = _model("skewq", metric)
    assert m.clamped_share(dat["x4"]) >= 0.5 and m.clamped_share(dat["plus1"]) >= 0.5 and m.clamped_share(dat["xq"]) < 0.5
    assert 0 < GROW_K[3] < 5000 and _capacity([CHUNK] * 4 + GROW_K[:3]) == CAP_AT_BASE < _capacity([CHUNK] * 4 + GROW_K)


# ---- the device -------------------------------------------------------------------------------------------------------------------


def _index(mf, metric, xb, prefilter, chunk=CHUNK):
    ix = mf.index_factory(xb.shape[1], "Flat", metric)
    ix.set_option("prefilter", prefilter)
    ix.set_option("cl_i8", 1)
    ix.set_option("flat_shadow", 0)
    for i0 in range(0, len(xb), chunk):
        ix.add(xb[i0 : i0 + chunk])
    return ix


def _same(a, b):
    (D1, I1), (D2, I2) = a, b
    return np.array_equal(I1, I2) and np.array_equal(D1.view(np.uint32), D2.view(np.uint32))


def _served(ix):
    return "%s store, kernel %s" % ("int8" if ix.get_stat("cl_store_i8") == 1 else "bf16", ix.last_kernel_info()["name"])


def _delta(ix, before):
    st = ix.collect_stats()
    return {k: st[k] - before[k] for k in st}


def _verify(mf, orc, ix, metric, xb, xq, k, want, what, ex=None, may_overflow=False):
    """search on ix: the store `want` ("int8" | "bf16") served it, on flat_bf16_collect_kernel -- unless the candidate stream overflowed,
    which only the cases that say so may do (the batch then ends on a fall-back kernel, named in the message) -- and the results are
    those of the exact f32 kernel on a fresh index of xb and, for the first 16 queries, of the oracle's BLAS branch; -> (results, the
    exact index, the message)"""
    before = ix.collect_stats()
    r = ix.search(xq, k)
    cs = _delta(ix, before)
    tag = "%s, k = %d, N = %d: served by %s, %d candidates for %d queries, %d overflows (model: %s)" % (
        what, k, len(xb), _served(ix), cs["candidates"], cs["queries"], cs["overflows"], want)  # fmt: skip
    print("\n" + tag)
    assert ix.get_stat("cl_store_i8") == (1 if want == "int8" else 0), tag
    if ix.last_kernel_info()["name"] != KERNEL:  # (an overflow the filter relieves itself -- the heaviest queries taken out, a second scan -- stays on it)
        assert may_overflow and cs["overflows"] > 0, tag
    ex = ex or _index(mf, metric, xb, 0)
    assert ex.ntotal == len(xb)
    re = ex.search(xq, k)
    assert ex.last_kernel_info()["name"] != KERNEL, tag
    assert _same(r, re), tag + ": differs from the exact f32 kernel"
    Do, Io = orc.flat_search(metric, xb, xq[:16], k, force_path=orc.PATH_BLAS)
    assert _same((r[0][:16], r[1][:16]), (Do, Io)), tag + ": differs from the oracle"
    return r, ex, tag


def _mname(metric):
    return "L2" if metric == L2 else "IP"


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("chunk", [1 << 30, 1000], ids=["one_add", "adds_of_1000"])
@pytest.mark.parametrize("d", NARROW)
def test_narrow_rows(mf, orc, d, chunk, metric):
    """17 <= d < 128: f32 rows of pitch 32, 64 or 128, int8 rows of pitch 128, the query fragments zero beyond d; k = 10 and k = 100
    (at d = 17 distances nearly tie: the heaviest candidate load); rows added at once, and in 1000-row calls through the staging slots"""
    key = "narrow:%d" % d
    dat, m = _data(key), _model(key, metric)
    xb, xq = dat["xb"], dat["xq"]
    i8 = _index(mf, metric, xb, 2, chunk)
    what = "uniform d = %d %s" % (d, _mname(metric))
    r, ex, _ = _verify(mf, orc, i8, metric, xb, xq, 10, m.decided(), what)
    assert i8.get_stat("cl_store_i8") == 1, what
    if metric == L2:
        assert [int(v) for v in r[1][: len(dat["on_rows"]), 0]] == [int(v) for v in dat["on_rows"]], what
    _verify(mf, orc, i8, metric, xb, xq, 100, m.decided(), what, ex)


SKEWED_ROWS = ["clustered", "offset", "colscale", "lattice", "sparse"]


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [128, 48])
@pytest.mark.parametrize("kind", SKEWED_ROWS)
def test_skewed_rows(mf, orc, kind, d, metric):
    """(a) clusters of sigma 0.05, queries near rows; (b) rows + 100: the centring absorbs the offset, the inner product's beta = <mu, y>
    may not fit the integer range; (c) column scales 1 ... 30; (d) a {-1, 0, 1} lattice with duplicated rows: ties at the k-th place,
    equal s_int everywhere (k = 10 and 100); (e) 90 % zeros -- on the store the model predicts"""
    key = "%s:%d" % (kind, d)
    dat, m = _data(key), _model(key, metric)
    xb, xq = dat["xb"], dat["xq"]
    i8 = _index(mf, metric, xb, 2)
    what = "(%s) %s rows d = %d %s [%s]" % ("abcde"[SKEWED_ROWS.index(kind)], kind, d, _mname(metric), m.describe())
    # (b): the bound carries the float32 rounding of the exact value, which grows with the UNCENTRED norms -- at an offset of 100 it is
    # wider than the spread of the distances, every row is a candidate and the batch ends on the fall-back: same results, slower
    _, ex, _ = _verify(mf, orc, i8, metric, xb, xq, 10, m.decided(), what, may_overflow=kind == "offset")
    assert i8.get_stat("flat_outlier_rows") == m.outlier_rows().size, what
    if kind == "lattice":
        _verify(mf, orc, i8, metric, xb, xq, 100, m.decided(), what, ex)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [128, 48])
def test_identical_rows_decline_the_store(mf, orc, d, metric):
    """(f) amax = 0: there is nothing to scale by; every distance ties, so whichever kernel ends up serving the batch returns FAISS's choice among them (L2: rows 0 ... 9)"""
    key = "identical:%d" % d
    dat, m = _data(key), _model(key, metric)
    assert m.decided() == "bf16" and m.amax == 0.0
    i8 = _index(mf, metric, dat["xb"], 2)
    r, _, _ = _verify(mf, orc, i8, metric, dat["xb"], dat["xq"], 10, "bf16", "(f) identical rows d = %d %s" % (d, _mname(metric)), may_overflow=True)
    if metric == L2:  # (inner product: FAISS's heap decides among equal scores, not the row number -- the oracle's order was asserted above)
        assert np.array_equal(r[1], np.tile(np.arange(10), (NQ, 1))), _served(i8)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_spiky_column_at_d_48(mf, orc, metric):
    """(g) one column of 4000 x the others' span, in a narrow row"""
    dat, m = _data("spiky:48"), _model("spiky:48", metric)
    assert m.decided() == "bf16"
    i8 = _index(mf, metric, dat["xb"], 2)
    _verify(mf, orc, i8, metric, dat["xb"], dat["xq"], 10, "bf16", "(g) spiky column d = 48 %s [%s]" % (_mname(metric), m.describe()),
            may_overflow=True)  # (the bf16 store's bound drowns in that column too: the batch may end on the fall-back)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("skew", ["x4", "plus1"])
def test_skewed_query_batch(mf, orc, skew, metric):
    """(h) the whole batch scaled by four about the rows' mean, (i) offset by one per component: most queries clamp at +-128 sa, their E
    widens, the stream may overflow -- same results; an ordinary batch behind it is exact on whichever path the skip counter gives it,
    and within 64 further searches the coarse filter serves ordinary batches again"""
    dat, m = _data("skewq"), _model("skewq", metric)
    xb, xq, bad = dat["xb"], dat["xq"], dat[skew]
    assert m.decided() == "int8" and m.clamped_share(bad) >= 0.5
    i8 = _index(mf, metric, xb, 2)
    what = "(%s) queries %s %s, %.0f %% of them clamped" % ("h" if skew == "x4" else "i", skew, _mname(metric), 100 * m.clamped_share(bad))
    before = i8.collect_stats()
    r = i8.search(bad, 10)
    cs = _delta(i8, before)
    what += ": %d candidates for %d queries, %d overflows, served by %s" % (cs["candidates"], cs["queries"], cs["overflows"], _served(i8))
    print("\n" + what)
    assert i8.get_stat("cl_store_i8") == 1, what
    if cs["overflows"] == 0:
        assert i8.last_kernel_info()["name"] == KERNEL, what
    ex = _index(mf, metric, xb, 0)
    assert _same(r, ex.search(bad, 10)), what + ": differs from the exact f32 kernel"
    Do, Io = orc.flat_search(metric, xb, bad[:16], 10, force_path=orc.PATH_BLAS)
    assert _same((r[0][:16], r[1][:16]), (Do, Io)), what + ": differs from the oracle"
    re = ex.search(xq, 10)
    assert _same(i8.search(xq, 10), re), what + "; the ordinary batch behind it (%s) differs from the exact f32 kernel" % _served(i8)
    for further in range(65):
        if i8.last_kernel_info()["name"] == KERNEL:
            break
        assert _same(i8.search(xq, 10), re), what + "; ordinary batch %d behind it (%s)" % (further + 2, _served(i8))
    assert i8.last_kernel_info()["name"] == KERNEL and i8.get_stat("cl_store_i8") == 1, what + "; 64 searches later: " + _served(i8)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_queries_that_are_not_finite(mf, orc, metric):
    """(j) 290 ordinary queries and ten with a NaN, an infinity or +-1e30 in one component: their bound is not finite, they are re-run on
    the exact kernel, the others stay on the int8 store"""
    dat, m = _data("skewq"), _model("skewq", metric)
    i8 = _index(mf, metric, dat["xb"], 2)
    _verify(mf, orc, i8, metric, dat["xb"], dat["bad"], 10, m.decided(), "(j) ten non-finite queries %s" % _mname(metric))
    assert i8.prefilter_stats()["fallback_queries"] >= 10


def _grow(mf, orc, key, metric, what, k=10, scale_on=1.0, may_overflow=False):
    """search at every stage of a grown index: sixteen queries sit on the rows added last (scale_on: a hair off them); yields per stage
    (index, model, rows so far, queries, results)"""
    dat, m = _data(key), _model(key, metric)
    stages = dat["stages"]
    i8 = _index(mf, metric, dat["xb"][: stages[0]], 2)
    prev = 0
    for n in stages:
        if n > stages[0]:
            i8.add(dat["xb"][prev:n])
        xb = dat["xb"][:n]
        rows = _spread(prev, n - 1)
        xq = dat["xq"].copy()
        xq[: len(rows)] = xb[rows] * np.float32(scale_on if prev else 1.0)
        want = m.decided(n) if n >= m.n_i8 else "bf16"
        r, _, _ = _verify(mf, orc, i8, metric, xb, xq, k, want, "%s %s, %d rows behind the first search" % (what, _mname(metric), n - stages[0]),
                          may_overflow=may_overflow)
        if metric == L2:
            assert [int(v) for v in r[1][: len(rows), 0]] == [int(v) for v in rows], what
        yield i8, m, xb, xq, r
        prev = n


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_growth_by_a_few_rows_and_past_the_capacity(mf, orc, metric):
    """(k) + 1, + 127, + 129 rows, then the smallest count that passes the capacity the store was allocated for (ensure_i8_rows'
    reallocate-and-copy branch): searched on the int8 store before and after each"""
    seen = [i8.get_stat("cl_store_i8") for i8, *_ in _grow(mf, orc, "k", metric, "(k) uniform rows added")]
    assert seen == [1] * 5


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_growth_by_rows_that_clamp(mf, orc, metric):
    """(l) 64 rows three times as far from the mean: they clamp, the store stays int8 (only the range check is repeated for later rows)
    -- and its residual maximum, now a clamped row's, widens every query's E until the stream overflows: same results, on the fall-back.
    (q) then cl_i8 0 -> 1 -> 0: the same results on either store, and the bf16 store, whose residual the new rows hardly move, gets the
    batch back onto the coarse filter once the skip counter has run out"""
    for i8, m, xb, xq, r in _grow(mf, orc, "l", metric, "(l) rows x 3 about the mean added", may_overflow=True):
        pass
    assert i8.get_stat("cl_store_i8") == 1
    for v in (0, 1, 0):
        i8.set_option("cl_i8", v)
        for further in range(66):
            assert _same(i8.search(xq, 10), r), "(q) cl_i8 = %d, search %d: served by %s" % (v, further, _served(i8))
            assert i8.get_stat("cl_store_i8") == v, "(q) cl_i8 = %d: served by %s" % (v, _served(i8))
            if v == 1 or i8.last_kernel_info()["name"] == KERNEL:
                break
        assert v == 1 or i8.last_kernel_info()["name"] == KERNEL, "(q) cl_i8 = 0, 66 searches: served by %s" % _served(i8)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_growth_that_breaks_the_integer_range(mf, orc, metric):
    """(m) 64 rows whose beta_int no longer fits 2^23 - d 2^14 yet stay below the outlier threshold: the int8 store is dropped, the bf16
    store serves, the results stay exact"""
    seen = []
    for i8, *_ in _grow(mf, orc, "m:%d" % metric, metric, "(m) rows past the integer range added"):
        seen.append(i8.get_stat("cl_store_i8"))
        assert i8.get_stat("flat_outlier_rows") == 0
    assert seen == [1, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_growth_by_outlier_rows(mf, orc, metric):
    """(n) three rows of 100 x the usual norm arrive after the store was built: kept out of it, appended to every query's candidates, found
    by the queries that sit on them"""
    for i8, m, xb, xq, r in _grow(mf, orc, "n", metric, "(n) outlier rows added", scale_on=1.001):
        assert i8.get_stat("flat_outlier_rows") == m.outlier_rows(len(xb)).size, _served(i8)
    assert i8.get_stat("flat_outlier_rows") == 3 and i8.get_stat("cl_store_i8") == 1


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_growth_of_an_index_first_searched_when_small(mf, orc, metric):
    """(o) the centre is fixed at 70 000 rows and there is no outlier threshold; grown to BASE + 1000 rows, two of them 100 x the usual
    norm: whichever store the model predicts for that, the results are exact"""
    for i8, m, xb, xq, r in _grow(mf, orc, "o", metric, "(o) first searched at 70 000 rows", may_overflow=True):
        assert i8.get_stat("flat_outlier_rows") == 0
    assert len(xb) == BASE + 1000


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("order", [("spiky:48", "uniform:48"), ("uniform:48", "spiky:48")], ids=["declined_then_int8", "int8_then_declined"])
def test_the_decision_is_taken_afresh_for_new_contents(mf, orc, order, metric):
    """(p) an index emptied and filled with other data decides again: spiky rows (declined), then uniform rows (int8), and the reverse"""
    i8 = None
    for key in order:
        dat, m = _data(key), _model(key, metric)
        if i8 is None:
            i8 = _index(mf, metric, dat["xb"], 2)
        else:
            assert i8.remove_ids(("batch", np.arange(i8.ntotal, dtype=np.int64))) == len(xb) and i8.ntotal == 0
            for i0 in range(0, len(dat["xb"]), CHUNK):
                i8.add(dat["xb"][i0 : i0 + CHUNK])
        xb = dat["xb"]
        _verify(mf, orc, i8, metric, xb, dat["xq"], 10, m.decided(), "(p) %s %s" % (" then ".join(order[: order.index(key) + 1]), _mname(metric)),
                may_overflow=key.startswith("spiky"))
