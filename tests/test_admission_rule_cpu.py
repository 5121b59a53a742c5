"""The admission rule of the scanning coded kinds (tests/admission_rule.py) against a literal replay of FAISS's heap, the direct chain
evaluations of the models against their oracle-derived versions, and the preconditions of tests/test_coded_nonfinite_gpu.py -- everything
about the non-finite cases that is decidable without a GPU."""
import numpy as np
import pytest

import nonfinite_cases as nfc
import pq_reference as pqr
import sq_reference as sqr
from admission_rule import admitted
from oracle import oracle as orc

L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
F = np.float32
FLT_MAX = F(np.finfo(np.float32).max)
NAN_POS, NAN_NEG = np.array([0x7FC00000, 0xFFC00000], dtype=np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------------------ FAISS's heap, literally
def faiss_heap(metric, row, k):
    """HeapResultHandler over one query's scores in row order (faiss/utils/Heap.h): the heap starts full of (neutral, -1); add_result calls
    replace_top iff C::cmp(top, dis) -- CMax (L2): top > dis, CMin (inner product): top < dis; heap_reorder pops everything, best last to front,
    and drops the -1 entries.  Nodes compare by (value, id) as C::cmp2 does.  -> (D [k], I [k])"""
    l2 = metric == L2
    neutral = FLT_MAX if l2 else -FLT_MAX

    def nearer_root(a, ia, b, ib):  # cmp2: a is worse than b
        return (a > b or (a == b and ia > ib)) if l2 else (a < b or (a == b and ia < ib))

    def sift(hv, hi, n, v, vid):  # replace the root of the first n nodes with (v, vid)
        i = 1
        while 2 * i <= n:
            c = 2 * i
            if c + 1 <= n and nearer_root(hv[c], hi[c], hv[c - 1], hi[c - 1]):
                c += 1
            if not nearer_root(hv[c - 1], hi[c - 1], v, vid):
                break
            hv[i - 1], hi[i - 1] = hv[c - 1], hi[c - 1]
            i = c
        hv[i - 1], hi[i - 1] = v, vid

    hv, hi = [neutral] * k, [-1] * k
    for j, dis in enumerate(row):
        if (hv[0] > dis) if l2 else (hv[0] < dis):  # accepts: an f32 comparison, false for NaN
            sift(hv, hi, k, dis, j)
    out = []
    for n in range(k, 0, -1):  # pop: worst first
        out.append((hv[0], hi[0]))
        if n > 1:
            sift(hv, hi, n - 1, hv[n - 1], hi[n - 1])
    out = [e for e in reversed(out) if e[1] != -1]
    out += [(neutral, -1)] * (k - len(out))
    return np.array([e[0] for e in out], dtype=np.float32), np.array([e[1] for e in out], dtype=np.int64)


def rule_then_sort(metric, row, k):
    """the helper, then the pure order: (value, row) -- what the four models do"""
    l2 = metric == L2
    rows = np.nonzero(admitted(metric, row))[0]
    order = rows[np.lexsort((rows, row[rows] if l2 else -row[rows]))][:k]
    D = np.full(k, FLT_MAX if l2 else -FLT_MAX, dtype=np.float32)
    I = np.full(k, -1, dtype=np.int64)
    D[: order.size], I[: order.size] = row[order], order
    return D, I


NEXT_BELOW_MAX = np.nextafter(FLT_MAX, F(0))
CRAFTED = {
    # (+0 and -0 sit in different rows: they are EQUAL floats, and which of two tied values prints first is the labels' matter below)
    "every class": [3.5, NAN_POS, 0.25, np.inf, FLT_MAX, 0.0, -np.inf, NAN_NEG, -FLT_MAX, NEXT_BELOW_MAX, -NEXT_BELOW_MAX, -7.25, 1e-45, 2.0, -1e30, 1e30],
    "nothing admissible under L2": [np.inf, NAN_POS, FLT_MAX, NAN_NEG, np.inf, FLT_MAX],
    "nothing admissible under inner product": [-np.inf, NAN_NEG, -FLT_MAX, NAN_POS, -np.inf],
    "fewer than k admissible": [NAN_NEG, np.inf, -np.inf, 5.0, NAN_POS, FLT_MAX, -FLT_MAX, -3.0, np.inf, -np.inf, NAN_POS, NAN_NEG, FLT_MAX, -FLT_MAX],
    "NaN first, then more than k finite": [NAN_NEG, NAN_POS] + [float(v) for v in np.random.default_rng(3).permutation(40) - 20.5] + [np.inf, -np.inf],
    "ties at both infinities": [np.inf, 1.0, np.inf, -np.inf, 2.0, -np.inf, np.inf, NAN_POS, -np.inf],
    "negative zero": [1.0, -0.0, NAN_NEG, -1.0, np.inf, -np.inf, FLT_MAX, -FLT_MAX],
    "only the neutral elements": [FLT_MAX, -FLT_MAX, FLT_MAX, -FLT_MAX],
}


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_rule_plus_sort_prints_what_the_heap_prints(name, metric):
    row = np.array(CRAFTED[name], dtype=np.float32)
    for k in (1, 3, 10, len(row) + 2):
        Dh, Ih = faiss_heap(metric, row, k)
        Dm, Im = rule_then_sort(metric, row, k)
        assert np.array_equal(Dh.view(np.uint32), Dm.view(np.uint32)), (name, k, Dh, Dm)
        live = Ih >= 0
        assert np.array_equal(live, Im >= 0)
        assert not np.isnan(Dh).any()
        if np.unique(Dh[live]).size == live.sum():  # distinct values: the labels are determined (under ties the coded kinds keep the pure order)
            assert np.array_equal(Ih, Im), (name, k, Ih, Im)


def test_the_crafted_rows_hold_every_class_and_both_counts():
    row = np.array(CRAFTED["every class"], dtype=np.float32)
    bits = set(np.concatenate([np.array(v, dtype=np.float32) for v in CRAFTED.values()]).view(np.uint32).tolist())
    for want in (0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000000, 0x80000000):
        assert want in bits
    assert nfc.classes(row) == {"nan", "+inf", "-inf", "finite"}
    for metric in (L2, IP):
        assert admitted(metric, row).sum() > 10  # more than k = 10
        few = admitted(metric, np.array(CRAFTED["fewer than k admissible"], dtype=np.float32)).sum()
        assert 1 <= few < 10
    assert not admitted(L2, np.array(CRAFTED["nothing admissible under L2"], dtype=np.float32)).any()
    assert not admitted(IP, np.array(CRAFTED["nothing admissible under inner product"], dtype=np.float32)).any()


def test_the_helper_agrees_with_the_oracle_heap_on_the_crafted_rows():
    """the oracle's own heap (oracle/orc_core.c, what the Flat kinds are held to) over the same rows, through its exported primitives"""
    L = orc.lib()
    for name, vals in CRAFTED.items():
        row = np.array(vals, dtype=np.float32)
        for metric in (L2, IP):
            for k in (1, 10):
                Dh, Ih = faiss_heap(metric, row, k)
                hv, hi = np.empty(k, dtype=np.float32), np.empty(k, dtype=np.int64)
                is_max = 1 if metric == L2 else 0
                L.orc_heap_init(k, hv.ctypes.data, hi.ctypes.data, is_max)
                for j, dis in enumerate(row):
                    if (hv[0] > dis) if metric == L2 else (hv[0] < dis):
                        L.orc_heap_replace_top(k, hv.ctypes.data, hi.ctypes.data, is_max, float(dis), j)
                L.orc_heap_reorder(k, hv.ctypes.data, hi.ctypes.data, is_max)
                assert np.array_equal(hv.view(np.uint32), Dh.view(np.uint32)) and np.array_equal(hi, Ih), (name, metric, k)


# ------------------------------------------------------------------------------------------------ the models' selects apply it
def test_the_flat_selects_pad_what_the_rule_refuses():
    row = np.array([CRAFTED["every class"], CRAFTED["every class"][::-1]], dtype=np.float32)
    ids = np.arange(row.shape[1], dtype=np.int64) * 5 + 100
    for metric in (L2, IP):
        for k in (1, 10, 20):
            for select in (pqr.select, sqr.sq_select):
                D, I = select(row, k, metric, labels=ids)
                for q in range(2):
                    Dm, Im = rule_then_sort(metric, row[q], k)
                    assert np.array_equal(D[q].view(np.uint32), Dm.view(np.uint32))
                    assert np.array_equal(I[q], np.where(Im >= 0, ids[np.maximum(Im, 0)], -1))


# ------------------------------------------------------------------------------------------------ direct chains == oracle-derived, finite input
@pytest.mark.parametrize("metric", [L2, IP])
def test_direct_tables_and_chains_equal_the_oracle_derived_ones_on_finite_input(metric):
    rng = np.random.default_rng(5 + metric)
    for M, dsub in ((8, 4), (80, 2), (3, 1), (2, 24)):
        cb = pqr.synthetic_codebooks(rng, M, dsub)
        xq = rng.standard_normal((9, M * dsub)).astype(np.float32)
        xq[3] *= 1e15  # large and finite: squares near 1e30, sums far below FLT_MAX
        xq[4] *= 1e-30
        assert np.array_equal(pqr.tables(cb, xq, metric).view(np.uint32), pqr.tables_by_search(cb, xq, metric).view(np.uint32))
    for d in (1, 20, 33):
        rows = rng.standard_normal((500, d)).astype(np.float32)
        xq = rng.standard_normal((7, d)).astype(np.float32)
        xq[2] *= 1e15
        assert np.array_equal(sqr.chains(metric, rows, xq).view(np.uint32), sqr.chains_by_search(metric, rows, xq).view(np.uint32))


def test_the_oracle_derived_tables_cannot_serve_a_non_finite_query():
    """why tables() evaluates its chain directly: the k = 256 search applies the rule in question to the table's entries"""
    rng = np.random.default_rng(8)
    cb = pqr.synthetic_codebooks(rng, 2, 4)
    xq = rng.standard_normal((2, 8)).astype(np.float32)
    xq[1, 5] = np.nan
    with pytest.raises(AssertionError):
        pqr.tables_by_search(cb, xq, L2)
    T = pqr.tables(cb, xq, L2)
    assert np.isfinite(T[0]).all() and np.isfinite(T[1, 0]).all() and np.isnan(T[1, 1]).all()


# ------------------------------------------------------------------------------------------------ preconditions of the GPU cases
@pytest.mark.parametrize("kind", sorted(nfc.KINDS))
def test_the_hostile_queries_are_what_they_are_named(kind):
    c = nfc.inputs(kind)
    xq, bits = c["xq"], c["xq"].view(np.uint32)
    assert xq.shape[0] == nfc.NQ + (2 if c["ivf"] else 0) and nfc.NQ == 17
    assert bits[nfc.Q_NAN_POS, nfc.HOSTILE] == 0x7FC00000 and bits[nfc.Q_NAN_NEG, nfc.HOSTILE] == 0xFFC00000
    assert xq[nfc.Q_INF_POS, nfc.HOSTILE] == np.inf and xq[nfc.Q_INF_NEG, nfc.HOSTILE] == -np.inf
    for q in (nfc.Q_NAN_POS, nfc.Q_NAN_NEG, nfc.Q_INF_POS, nfc.Q_INF_NEG):
        assert np.isfinite(np.delete(xq[q], nfc.HOSTILE)).all()
    assert (xq[nfc.Q_1E30] == F(1e30)).all() and (xq[nfc.Q_SQUARES] == F(1.5e19)).all()
    with np.errstate(over="ignore"):
        s = F(1.5e19) * F(1.5e19)
        assert np.isfinite(s) and np.isinf(s + s)
    for q in nfc.COPIES:
        assert np.array_equal(bits[q], bits[0])
    hostile = {nfc.Q_NAN_POS, nfc.Q_NAN_NEG, nfc.Q_INF_POS, nfc.Q_INF_NEG, nfc.Q_1E30, nfc.Q_SQUARES, nfc.Q_NO_COARSE, nfc.Q_FINE_BEYOND}
    for q in range(xq.shape[0]):
        assert np.isfinite(xq[q]).all() and np.abs(xq[q]).max() < 10 or q in hostile
    assert np.isfinite(c["xb"]).all() and np.abs(c["xb"]).max() < 16  # rows: finite, ordinary
    assert c["xb"].shape[0] == (nfc.N_IVF if c["ivf"] else nfc.N_FLAT) and nfc.N_FLAT == 2 * 8192 + 77


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("kind", sorted(nfc.KINDS))
def test_no_gpu_case_is_vacuous(kind, metric):
    c = nfc.inputs(kind)
    rows = nfc.score_rows(kind, metric)
    want = nfc.EXPECTED_CLASSES[("ivf" if c["ivf"] else "flat", metric)]
    for q, cls in want.items():
        assert nfc.classes(rows[q][0]) == cls, (kind, metric, q, nfc.classes(rows[q][0]))
    for q in nfc.CONTROLS + (8, 15):
        assert nfc.classes(rows[q][0]) == {"finite"} and np.abs(rows[q][0]).max() < 1e6
    if c["ivf"]:
        P = nfc.scores(kind, metric)[0]
        assert (P[nfc.Q_NO_COARSE] == -1).all() and (P[nfc.Q_NAN_POS] == -1).all() and (P[nfc.Q_NAN_NEG] == -1).all()
        assert (P[0] >= 0).all()
        sizes = [ids.size for ids, _ in nfc.scores(kind, metric)[1]]
        assert max(sizes) > nfc.R and sum(sizes) == nfc.N_IVF  # one list exceeds a window
        if metric == IP:
            assert (P[nfc.Q_FINE_BEYOND] >= 0).all()  # finite coarse values ...
            beyond = nfc.classes(rows[nfc.Q_FINE_BEYOND][0])
            assert beyond and beyond <= {"+inf", "-inf"}  # ... and every fine score beyond FLT_MAX
            assert P[nfc.Q_INF_POS].tolist() == [0, -1] and P[nfc.Q_INF_NEG].tolist() == [1, -1]
    k = 10
    n_adm = [int(admitted(metric, v).sum()) for v, _ in rows]
    assert min(n_adm) == 0
    assert all(n_adm[q] == 0 for q in (nfc.Q_NAN_POS, nfc.Q_NAN_NEG))
    both_sides = [q for q, (v, pos) in enumerate(rows) if n_adm[q] >= k and admitted(metric, v)[pos < nfc.R].any() and admitted(metric, v)[pos >= nfc.R].any()]
    assert set(nfc.CONTROLS) <= set(both_sides)
    if metric == IP:  # (under L2 a query's rows are admissible all or none: tests/nonfinite_cases.py)
        assert n_adm[nfc.Q_INF_POS] == len(c["planted"]) and 1 <= n_adm[nfc.Q_INF_POS] <= k - 1
        v, pos = rows[nfc.Q_INF_POS]
        adm_pos = pos[admitted(metric, v)]
        assert (adm_pos < nfc.R).any() and (adm_pos >= nfc.R).any()  # the bound is still open when the later range / window brings the rest
        assert nfc.Q_INF_NEG in both_sides and n_adm[nfc.Q_INF_NEG] > 1000
    # the answers themselves: padded where the rule says so, the copies equal to q0
    for kk in nfc.KS:
        D, I = nfc.expected(kind, metric, kk)
        assert not np.isnan(D).any()
        for q in range(len(rows)):
            live = min(n_adm[q], kk)
            assert (I[q, :live] >= 0).all() and (I[q, live:] == -1).all()
            assert (D[q, live:] == (FLT_MAX if metric == L2 else -FLT_MAX)).all()
        for q in nfc.COPIES:
            assert np.array_equal(I[q], I[0]) and np.array_equal(D[q].view(np.uint32), D[0].view(np.uint32))
    if metric == IP:
        D, I = nfc.expected(kind, metric, 10)
        assert (D[nfc.Q_INF_POS, : len(c["planted"])] == np.inf).all() and (D[nfc.Q_INF_NEG] == np.inf).all()
        if not c["ivf"]:  # +inf rows come first, in row order
            assert I[nfc.Q_INF_POS, : len(c["planted"])].tolist() == list(c["planted"])
            assert (np.diff(I[nfc.Q_INF_NEG]) > 0).all()


@pytest.mark.parametrize("kind", nfc.IDMAP_KINDS)
def test_idmap_cases_print_ids_that_are_no_row_numbers(kind):
    base = nfc.base_kind(kind)
    ids = nfc.inputs(base)["ids"]
    assert ids.min() > ids.size  # no id can be mistaken for a row number
    D, I = nfc.expected(kind, IP, 10)
    Db, Ib = nfc.expected(base, IP, 10)
    assert np.array_equal(D.view(np.uint32), Db.view(np.uint32))
    assert np.array_equal(I, np.where(Ib >= 0, ids[np.maximum(Ib, 0)], -1)) and (I == -1).any() and (I >= 0).any()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("kind", sorted(nfc.N_OVERFLOW))
def test_best_last_rows_improve_for_the_controls(kind, metric):
    """the overflow cases' premise: nearly every row of the second range / window beats the k-th best of the first R rows -- more candidates
    than a bucket of R entries holds"""
    s = nfc.overflow_scores(kind, metric)
    want = nfc.EXPECTED_CLASSES[("flat", metric)]
    for q, cls in want.items():
        assert nfc.classes(s[q]) == cls, (kind, metric, q)
    for q in nfc.CONTROLS:
        key = s[q] if metric == L2 else -s[q]
        bound = np.sort(key[: nfc.R])[9]
        assert (key[nfc.R : 3 * nfc.R] < bound).sum() > nfc.R


# ------------------------------------------------------------------------------------------------ the device's form of the rule
def _key(v, descending):
    """csrc/pq_kernels.h pq_key restated on uint32: smaller key = better entry"""
    b = np.asarray(v, dtype=np.float32).view(np.uint32)
    a = b ^ np.where(b >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
    return ~a if descending else a


def _bound_value(thr, descending):
    """pq_bound_value: pq_unkey(thr), negated (a sign flip) under inner product"""
    a = ~np.asarray(thr, dtype=np.uint32) if descending else np.asarray(thr, dtype=np.uint32)
    b = np.where(a >> 31, a ^ np.uint32(0x80000000), ~a)
    return (b ^ np.uint32(0x80000000 if descending else 0)).astype(np.uint32).view(np.float32)


def _beats(v, bound_value, descending):
    """pq_beats: the value, sign-flipped under inner product, below the bound's value -- an f32 comparison"""
    w = (np.asarray(v, dtype=np.float32).view(np.uint32) ^ np.uint32(0x80000000 if descending else 0)).view(np.float32)
    with np.errstate(invalid="ignore"):
        return w < bound_value


@pytest.mark.parametrize("metric", [L2, IP])
def test_the_open_bound_and_the_value_test_are_the_rule(metric):
    """a value beats PQ_OPEN_BOUND iff admitted(); it beats the bound a list member's key stands for iff it is strictly better than that
    member -- which is "its key is below" for every pair but +0.0 against -0.0; a bound of 0 is beaten by nothing: on the crafted rows, on
    every exponent with extreme mantissas and both signs, and on random bit patterns (NaN payloads included)"""
    OPEN = np.array([0xFF7FFFFF], dtype=np.uint32)
    desc = metric == IP
    assert _key(np.array([FLT_MAX if metric == L2 else -FLT_MAX], dtype=np.float32), desc)[0] == OPEN[0]
    assert _bound_value(OPEN, desc).view(np.uint32)[0] == 0x7F7FFFFF  # FLT_MAX on the ascending side under both metrics
    rng = np.random.default_rng(12)
    exps = (np.arange(256, dtype=np.uint32) << 23)[:, None] | np.array([0, 1, 0x400000, 0x7FFFFF], dtype=np.uint32)[None, :]
    bits = np.concatenate([exps.ravel(), exps.ravel() | np.uint32(0x80000000), rng.integers(0, 2**32, 200000, dtype=np.uint64).astype(np.uint32)])
    v = np.concatenate([bits.view(np.float32)] + [np.array(r, dtype=np.float32) for r in CRAFTED.values()])
    adm = admitted(metric, v)
    assert np.array_equal(_beats(v, _bound_value(OPEN, desc), desc), adm)
    assert np.isnan(v).sum() > 500 and not adm[np.isnan(v)].any()
    assert not _beats(v, _bound_value(np.zeros(1, dtype=np.uint32), desc), desc).any()  # bound 0: a slot without a query
    # against the bounds that list members leave: every admitted value in turn, paired with a shuffled copy
    a = v[adm]
    b = rng.permutation(a)
    better = (a < b) if metric == L2 else (a > b)
    got = _beats(a, _bound_value(_key(b, desc), desc), desc)
    assert np.array_equal(got, better)
    mixed_zero = (a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))
    assert np.array_equal(got[~mixed_zero], (_key(a, desc) < _key(b, desc))[~mixed_zero])
    assert np.array_equal(_bound_value(_key(b, desc), desc).view(np.uint32), (b.view(np.uint32) ^ np.uint32(0x80000000 if desc else 0)))
