"""The preconditions of tests/test_flat_nonfinite_gpu.py, asserted without a GPU on the oracle alone: every hostile case of
tests/flat_nonfinite_cases.py really holds the score classes it is named for, the admissible rows straddle a row-split boundary, the IVF
lists hold and omit the rows the cases say, and the oracle's answers are the admission rule plus a sort wherever no tie decides."""
import numpy as np
import pytest

import flat_nonfinite_cases as fc
from flat_nonfinite_cases import IP, L2, admitted, classes
from oracle import oracle as orc

NANQ = (fc.Q_NAN_POS, fc.Q_NAN_NEG)
INFQ = (fc.Q_INF_NEG, fc.Q_INF_POS)


def _best_first(metric, vals, rows, k):
    """the k best admitted (value, row) by value, equal values in row order"""
    order = np.argsort(vals if metric == L2 else -vals, kind="stable")[:k]
    return vals[order], rows[order]


def _check_against_sort(metric, s, rows, D, I, k, what):
    """s, rows: the scores of the rows a query scans and their labels; (D, I): the oracle's answer"""
    adm = admitted(metric, s)
    v, r = _best_first(metric, s[adm], rows[adm], k + 1)
    n = min(k, int(adm.sum()))
    assert (I[n:] == -1).all() and (D[n:] == fc.neutral(metric)).all(), what
    assert (I[:n] >= 0).all() and not np.isnan(D).any(), what
    assert np.array_equal(D[:n].view(np.uint32), v[:n].view(np.uint32)), what  # (the values of the k best do not depend on how ties fall)
    if len(np.unique(v)) == len(v):  # the k best and the first one left out are distinct: no tie decides
        assert np.array_equal(I[:n], r[:n]), what
        return 1
    return 0


@pytest.mark.parametrize("d", fc.DIMS)
def test_the_batch_and_the_rows_are_what_the_cases_say(d):
    fin, hos = fc.flat_inputs("finite", d), fc.flat_inputs("hostile", d)
    assert fin["xb"].shape == hos["xb"].shape == (fc.N, d) and fin["xq"].shape == (fc.NQ, d) and np.array_equal(fin["xq"], hos["xq"], equal_nan=True)
    assert not fin["xb"].flags.writeable and not fin["xq"].flags.writeable
    xq, bits = fin["xq"], fin["xq"].view(np.uint32)
    assert bits[fc.Q_NAN_POS, fc.H] == 0x7FC00000 and bits[fc.Q_NAN_NEG, fc.H] == 0xFFC00000
    assert xq[fc.Q_INF_POS, fc.H] == np.inf and xq[fc.Q_INF_NEG, fc.H] == -np.inf
    assert xq[fc.Q_ZERO, fc.H] == 0.0 and xq[fc.Q_POS, fc.H] > 0 and xq[fc.Q_NEG, fc.H] < 0
    assert (xq[fc.Q_1E30] == np.float32(1e30)).all() and (xq[fc.Q_SQUARES] == np.float32(1.5e19)).all()
    for c in fc.COPIES:
        assert np.array_equal(xq[c].view(np.uint32), xq[0].view(np.uint32))
    finite_q = [q for q in range(fc.NQ) if q not in fc.HOSTILE_QUERIES]
    assert np.isfinite(xq[finite_q]).all() and set(fc.CONTROLS) <= set(finite_q)
    assert 0 in fc.CONTROLS and sum(q in fc.HOSTILE_QUERIES for q in range(3)) == 2  # the streaming kernel's batch: one control, two hostile
    assert set(fc.HOSTILE_QUERIES) <= set(range(7)) | {fc.Q_POS, fc.Q_NEG, fc.Q_1E30, fc.Q_SQUARES} and max(fc.HOSTILE_QUERIES) < 12
    # the ordinary rows: H is exactly 0 or negative, at about 30 : 70; only the planted rows are positive
    assert np.isfinite(fin["xb"]).all()
    col = fin["xb"][:, fc.H]
    assert sorted(np.flatnonzero(col > 0)) == sorted(fc.PLANTED) and 1 <= len(fc.PLANTED) <= fc.K - 1
    assert 0.25 < (col == 0).mean() < 0.35 and (col[col < 0] <= -0.25).all()
    # the hostile rows: three of each kind, around the boundary and in the last partial tile of both geometries
    where = hos["hostile"]
    assert sorted(where) == sorted(fc.HOSTILE_KINDS)
    hb = hos["xb"].view(np.uint32)
    for kind, rows in where.items():
        assert rows[0] < fc.BOUNDARY <= rows[1] and rows[2] >= (fc.N // 256) * 256 and rows[2] >= (fc.N // 64) * 64 and fc.N % 64 and fc.N % 256
    assert all(hb[r, fc.NAN_COL] == 0x7FC00000 for r in where["nan+"]) and all(hb[r, fc.NAN_COL] == 0xFFC00000 for r in where["nan-"])
    assert all(hos["xb"][r, fc.H] == np.inf for r in where["inf+"]) and all(hos["xb"][r, fc.H] == -np.inf for r in where["inf-"])
    assert all((hos["xb"][r] == np.float32(1e30)).all() for r in where["1e30"]) and all((hos["xb"][r] == np.float32(1.5e19)).all() for r in where["1.5e19"])
    assert all(0 < np.abs(hos["xb"][r]).max() < 1e-19 for r in where["tiny"])
    special = sorted(r for rows in where.values() for r in rows)
    others = np.setdiff1d(np.arange(fc.N), special)
    assert np.isfinite(hos["xb"][others]).all() and (hos["xb"][others, fc.H] <= 0).all()
    with np.errstate(all="ignore"):
        yn = orc.norms(hos["xb"])
    assert all(np.isinf(yn[r]) for kind in ("1e30", "1.5e19") for r in where[kind])  # each square of 1.5e19 is finite, their sum is not
    assert np.isfinite(np.float32(1.5e19) * np.float32(1.5e19))
    # the boundary starts a row split of the fused kernel's own plan at this N, and its selector keeps some hostile rows and drops others
    # (16 and 4 splits are what the plan picks here; the GPU test checks the count the kernel reports)
    assert fc.BOUNDARY % fc.split_rows(fc.N, d, 16 if d <= 128 else 4) == 0 and fc.split_rows(fc.N, d, 16 if d <= 128 else 4) < fc.N
    keep = fc.keep_rows("hostile", d)
    assert 0.35 < len(keep) / fc.N < 0.45 and 0 < np.isin(special, keep).sum() < len(special)


@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("branch", ["pair", "blas"])
def test_every_hostile_flat_query_holds_its_score_classes(branch, d):
    where = fc.flat_inputs("hostile", d)["hostile"]
    rows = {kind: list(r) for kind, r in where.items()}
    # ---- ordinary rows
    s = fc.flat_scores("finite", d, L2, branch)
    for q in NANQ:
        assert classes(s[q]) == {"nan"}
    for q in INFQ + (fc.Q_1E30, fc.Q_SQUARES):  # an L2 sum over ordinary rows is finite for every row or for none
        assert "+inf" in classes(s[q]) and not classes(s[q]) & {"finite", "-inf"}
    for q in (0, fc.Q_ZERO, fc.Q_POS, fc.Q_NEG):
        assert classes(s[q]) == {"finite"}
    s = fc.flat_scores("finite", d, IP, branch)
    for q in NANQ:
        assert classes(s[q]) == {"nan"}
    for q in INFQ:  # inf * (positive, negative, exactly 0)
        assert classes(s[q]) == {"+inf", "-inf", "nan"}
    for q in (fc.Q_1E30, fc.Q_SQUARES, 0):
        assert classes(s[q]) == {"finite"}
    # ---- hostile rows
    s = fc.flat_scores("hostile", d, L2, branch)
    for q in NANQ:
        assert classes(s[q]) == {"nan"}
    for q in (0, fc.Q_ZERO, fc.Q_POS, fc.Q_NEG):
        assert classes(s[q]) >= {"finite", "+inf", "nan"}
        assert np.isnan(s[q][rows["nan+"] + rows["nan-"]]).all()
        assert not admitted(L2, s[q][rows["inf+"] + rows["inf-"] + rows["1e30"] + rows["1.5e19"]]).any()
        assert np.isfinite(s[q][rows["tiny"]]).all()
    if branch == "pair":  # (1e30 - 1e30)^2 = 0: the 1e30 query has exactly its three rows; the norms formula gives inf - inf
        assert np.flatnonzero(admitted(L2, s[fc.Q_1E30])).tolist() == sorted(rows["1e30"]) and (s[fc.Q_1E30][rows["1e30"]] == 0).all()
    else:
        assert not admitted(L2, s[fc.Q_1E30]).any() and np.isnan(s[fc.Q_1E30][rows["1e30"]]).all()
    s = fc.flat_scores("hostile", d, IP, branch)
    for q in NANQ:
        assert classes(s[q]) == {"nan"}
    assert np.isnan(s[fc.Q_ZERO][rows["inf+"] + rows["inf-"]]).all() and "finite" in classes(s[fc.Q_ZERO])  # 0 * inf
    assert (s[fc.Q_POS][rows["inf+"]] == np.inf).all() and (s[fc.Q_POS][rows["inf-"]] == -np.inf).all()
    assert (s[fc.Q_NEG][rows["inf+"]] == -np.inf).all() and (s[fc.Q_NEG][rows["inf-"]] == np.inf).all()
    for q in (0, fc.Q_POS, fc.Q_NEG, fc.Q_1E30, fc.Q_SQUARES):
        assert classes(s[q]) == {"finite", "+inf", "-inf", "nan"}
    for q in INFQ:
        assert classes(s[q]) == {"+inf", "-inf", "nan"}


@pytest.mark.parametrize("d", fc.DIMS)
def test_admissible_rows_come_in_every_number_on_both_sides_of_the_boundary(d):
    """0, 1 ... k - 1 and >= k admissible rows at k = 10, and where there are some they lie before and behind the row-split boundary"""
    k = fc.K

    def sides(mask):
        r = np.flatnonzero(mask)
        return (r < fc.BOUNDARY).any() and (r >= fc.BOUNDARY).any()

    for case in fc.CASES:
        c = fc.flat_inputs(case, d)
        for branch in ("pair", "blas"):
            s = fc.flat_scores(case, d, IP, branch)
            few, many = admitted(IP, s[fc.Q_INF_POS]), admitted(IP, s[fc.Q_INF_NEG])
            assert np.flatnonzero(few).tolist() == sorted(c["planted"]) and 1 <= few.sum() <= k - 1 and sides(few)
            assert (s[fc.Q_INF_POS][few] == np.inf).all()
            assert many.sum() > 1000 and sides(many) and (s[fc.Q_INF_NEG][many] == np.inf).all()  # thousands, all tied at +inf
            assert not admitted(IP, s[fc.Q_NAN_POS]).any() and not admitted(IP, s[fc.Q_NAN_NEG]).any()
            assert admitted(IP, s[0]).sum() >= k
    s = fc.flat_scores("hostile", d, L2, "pair")
    few = admitted(L2, s[fc.Q_1E30])
    assert few.sum() == 3 and sides(few) and admitted(L2, s[0]).sum() >= k and not admitted(L2, s[fc.Q_NAN_POS]).any()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("case", fc.CASES)
@pytest.mark.parametrize("d", fc.DIMS)
def test_the_flat_oracle_is_the_admission_rule_plus_a_sort(d, case, metric):
    rows = np.arange(fc.N)
    decided = 0
    for nq, branch in ((fc.NQ, "blas"), (7, "pair")):
        s = fc.flat_scores(case, d, metric, branch)
        for k in (1, fc.K):
            D, I = fc.expected(case, metric, k, nq, d)
            for q in range(nq):
                decided += _check_against_sort(metric, s[q], rows, D[q], I[q], k, f"{case} d={d} metric={metric} {branch} k={k} q{q}")
    # (over ordinary rows most queries have no tie among their best; the hostile rows tie on purpose -- three rows at +inf under inner product
    # for every query with a non-zero H, the three rows times 1e-20 at one L2 value that beats most ordinary rows -- and there only the
    # oracle's heap says in which order they print)
    assert decided >= (fc.NQ if case == "finite" else 1)
    ids = fc.flat_inputs(case, d)["ids"]
    D, I = fc.expected(case, metric, fc.K, fc.NQ, d)
    Dm, Im = fc.expected(case, metric, fc.K, fc.NQ, d, idmap=True)
    assert np.array_equal(D.view(np.uint32), Dm.view(np.uint32)) and np.array_equal(np.where(I >= 0, ids[I], -1), Im)  # an empty slot stays -1


@pytest.mark.parametrize("d", fc.IVF_DIMS)
def test_the_ivf_lists_hold_and_omit_what_the_cases_say(d):
    # inner product
    c, o = fc.ivf_inputs(IP, d), fc.ivf_oracle(IP, d)
    l0, l1 = o.ivf_list(0)[0], o.ivf_list(1)[0]
    where = c["hostile"]
    nan_rows = list(where["nan+"]) + list(where["nan-"])
    assert o.ntotal == fc.N_IVF and len(l0) + len(l1) == fc.N_IVF - len(nan_rows)  # ntotal counts the NaN rows, the lists do not
    assert not np.isin(nan_rows, l0).any() and not np.isin(nan_rows, l1).any()
    assert np.isin(where["inf+"], l0).all() and np.isin(where["inf-"], l1).all() and np.isin(where["1e30"], l0).all() and np.isin(c["planted"], l0).all()
    assert min(len(l0), len(l1)) > 256 + 64
    for kind in ("inf+", "inf-", "1e30"):  # one among the first 256 arrivals of its list, one behind them
        l = l1 if kind == "inf-" else l0
        pos = [int(np.flatnonzero(l == r)[0]) for r in where[kind]]
        assert pos[0] < 256 <= pos[1], (kind, pos)
    P = fc.ivf_probes(IP, d)
    assert P[fc.Q_INF_POS].tolist() == [0, -1] and P[fc.Q_INF_NEG].tolist() == [1, -1] and P[fc.Q_ONE_PROBE].tolist() == [0, -1]
    for q in NANQ + (fc.Q_NO_COARSE,):
        assert P[q].tolist() == [-1, -1]
    for q in (fc.Q_ZERO, fc.Q_POS, fc.Q_NEG, fc.Q_FAR):
        assert sorted(P[q].tolist()) == [0, 1]
    with np.errstate(all="ignore"):
        s = orc.pair_chains(IP, c["xb"], c["xq"])
    infs = list(where["inf+"]) + list(where["inf-"])
    assert np.isnan(s[fc.Q_ZERO][infs]).all()  # NaN, +inf and -inf inside the scan
    assert (s[fc.Q_POS][list(where["inf+"])] == np.inf).all() and (s[fc.Q_POS][list(where["inf-"])] == -np.inf).all()
    assert (s[fc.Q_NEG][list(where["inf+"])] == -np.inf).all() and (s[fc.Q_NEG][list(where["inf-"])] == np.inf).all()
    assert {"+inf", "-inf", "finite"} <= classes(s[fc.Q_FAR])  # 3e38 times a component beyond +-1.13 overflows
    # L2
    c, o = fc.ivf_inputs(L2, d), fc.ivf_oracle(L2, d)
    l0, l1 = o.ivf_list(0)[0], o.ivf_list(1)[0]
    nan_rows = [r for rows in c["hostile"].values() for r in rows]
    assert o.ntotal == fc.N_IVF and len(l0) + len(l1) == fc.N_IVF - len(nan_rows) and not np.isin(nan_rows, np.concatenate([l0, l1])).any()
    assert min(len(l0), len(l1)) > 256 + 64 and np.isin(c["planted"], l0).all()
    pos = [int(np.flatnonzero(l0 == r)[0]) for r in c["planted"]]
    assert pos[0] < 256 <= pos[1]
    # the query that reaches the scan: both coarse values finite under the pair and the BLAS formula, list 1 first, then list 0 with its +inf rows
    far = c["xq"][fc.Q_FAR : fc.Q_FAR + 1]
    with np.errstate(all="ignore"):
        pair = orc.pair_chains(L2, c["cent"], far)[0]
        blas = (orc.norms(far)[0] + orc.norms(c["cent"])) - np.float32(2) * orc.pair_chains(IP, c["cent"], far)[0]
        fine = orc.pair_chains(L2, c["xb"], far)[0]
    assert np.isfinite(pair).all() and np.isfinite(blas).all() and pair[1] < pair[0] and blas[1] < blas[0]
    P = fc.ivf_probes(L2, d)
    assert P[fc.Q_FAR].tolist() == [1, 0] and P[fc.Q_ONE_PROBE].tolist() == [0, -1]
    assert (fine[list(c["planted"])] == np.inf).all() and np.isfinite(fine[np.concatenate([l0[~np.isin(l0, c["planted"])], l1])]).all()
    for q in NANQ + INFQ + (fc.Q_1E30, fc.Q_SQUARES, fc.Q_NO_COARSE):  # no finite coarse value: probed nowhere
        assert P[q].tolist() == [-1, -1]
    assert sum(P[q].tolist() == [1, 0] for q in range(fc.NQ_IVF)) >= 3 and sum(P[q].tolist() == [0, 1] for q in range(fc.NQ_IVF)) >= 3


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", fc.IVF_DIMS)
def test_the_ivf_oracle_is_the_admission_rule_plus_a_sort(d, metric):
    c, o = fc.ivf_inputs(metric, d), fc.ivf_oracle(metric, d)
    lists = [o.ivf_list(l) for l in range(2)]
    with np.errstate(all="ignore"):
        dis = [orc.pair_chains(metric, rows, c["xq"]) for _, rows in lists]
    decided = 0
    for nprobe in (1, 2):
        P = fc.ivf_probes(metric, d, nprobe)
        for k in (1, fc.K):
            D, I = fc.ivf_expected(metric, d, k, nprobe)
            for q in range(fc.NQ_IVF):
                ls = [l for l in P[q] if l >= 0]
                s = np.concatenate([dis[l][q] for l in ls]) if ls else np.empty(0, dtype=np.float32)
                ids = np.concatenate([lists[l][0] for l in ls]) if ls else np.empty(0, dtype=np.int64)
                # (the model's tie order is the row number, the oracle's the heap's: compared only where no tie decides)
                decided += _check_against_sort(metric, s, ids, D[q], I[q], k, f"IVF d={d} metric={metric} nprobe={nprobe} k={k} q{q}")
    assert decided >= 1
    Dm, Im = fc.ivf_expected(metric, d, fc.K, 2, idmap=True)
    D, I = fc.ivf_expected(metric, d, fc.K, 2)
    assert np.array_equal(D.view(np.uint32), Dm.view(np.uint32)) and np.array_equal(np.where(I >= 0, c["ids"][I], -1), Im)


@pytest.mark.parametrize("nlist,n,k,nprobe,ms", [(16, 20000, 10, 4, (1, 9)), (32, 40000, 33, 8, (1, 32, 33))])
def test_the_filter_cases_put_nan_rows_into_the_bound_sample(nlist, n, k, nprobe, ms):
    """m rows with +inf in H are the first arrivals of the list the hostile queries probe first, and score NaN against them.  With
    m = k - 1 a bound that counted them among the k best of the first 256 rows -- the best REAL sampled value -- would cut off true results:
    the oracle's answer holds rows strictly worse than that value for every hostile query"""
    for m in ms:
        c = fc.filter_inputs(IP, nlist, n, m)
        o, star = c["oracle"], c["planted_list"]
        ids, rows = o.ivf_list(star)
        assert ids[:m].tolist() == list(range(m)) and len(ids) > 256 and o.ntotal == n
        hostile = c["xq"][: fc.FILTER_HOSTILE]
        assert (hostile[:, fc.H] == 0).all() and np.isfinite(hostile).all()
        assert (orc.flat_search(IP, c["cent"], c["xq"], nprobe)[1][: fc.FILTER_HOSTILE, 0] == star).all()
        with np.errstate(all="ignore"):
            s = orc.pair_chains(IP, rows[:256], hostile)
        assert np.isnan(s[:, :m]).all() and np.isfinite(s[:, m:]).all()
        D, I = o.search(c["xq"], k, nprobe=nprobe)
        assert not np.isin(I[: fc.FILTER_HOSTILE], np.arange(m)).any() and (I[: fc.FILTER_HOSTILE] >= 0).all()
        assert (I[fc.FILTER_Q_NAN] == -1).all() and np.isfinite(c["xq"][fc.FILTER_Q_BIG]).all()
        if m == k - 1 and k > 32:  # (the frozen bound of lists beyond 32 entries; up to 32 the scan keeps its own running bound)
            cut = (D[: fc.FILTER_HOSTILE] < s[:, m:].max(1)[:, None]).sum(1)
            print("results a bound at the best sampled value would drop, per hostile query:", cut.tolist())
            assert (cut >= 1).all()
