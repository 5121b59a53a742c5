"""The non-finite search cases of the Flat-backed kinds -- Flat, IVF<n>,Flat and their IDMap variants -- and the oracle's answers to them:
inputs of tests/test_flat_nonfinite_gpu.py, whose preconditions tests/test_flat_nonfinite_cases_cpu.py asserts without a GPU.  A helper
module: nothing here is collected.  The admission rule and the score classes are those of admission_rule.py and nonfinite_cases.py.

Unlike the coded kinds these store raw f32 rows, so ROWS can be hostile too.  Component H = 5 carries the signs:

Flat, N = 20 077 rows, d in (20, 100, 160); case "finite" has ordinary rows only, case "hostile" adds seven kinds of row (HOSTILE_KINDS), each
just before row BOUNDARY, just after it and in the last partial tile:
  nan+ / nan-   component 2 = NaN 0x7FC00000 / 0xFFC00000 (through the integer view)
  inf+ / inf-   component H = +inf / -inf: a query with exactly 0 there scores 0 * inf
  1e30          every component 1e30                      1.5e19   every component 1.5e19 (a square is finite, two of them are not)
  tiny          an ordinary row times 1e-20
An ordinary row holds exactly 0.0 (about 30 %) or -(|noise| + 0.25) in H; only the PLANTED rows of case "finite" hold a positive value there.
BOUNDARY = 5120 starts a row split of flat_mfma_kernel in both geometries at this N (split_rows() below restates its plan; the GPU test checks
it against the split count the kernel reports).

The batch of 24 queries (FAISS's BLAS branch; its first 7 are the per-pair branch, its first 3 the streaming kernel):
  q0, q6, q23   finite controls, q6 and q23 copies of q0        q1   H = NaN 0x7FC00000        q3   H = NaN 0xFFC00000
  q2            H = -inf       q4   H = +inf                    q5   H exactly 0               q7   H = 2       q8   H = -2
  q9            every component 1e30                            q10  every component 1.5e19    the others finite
Under inner product q4 has exactly len(PLANTED) admissible rows in case "finite" (between 1 and k - 1 at k = 10) and exactly the nine hostile
rows with a positive H in case "hostile", on both sides of BOUNDARY; q2 has thousands, all tied at +inf; q1 and q3 have none.

IVF2,Flat under inner product, centroids +-0.5 (nonfinite_cases.centroids): a row with +inf in H goes to list 0, one with -inf to list 1, a
NaN row to no list (ntotal counts it), a 1e30 row to list 0.  q5 / q7 / q8 score NaN / +inf / -inf against the inf rows INSIDE the scan.
IVF2,Flat under L2, centroids c0 = 0 and c1 = -1e19 e_H: rows near c0, rows at c1 + u 1e18 e_H, two rows at +1.4e19 e_H in list 0 (coarse value
1.96e38 to c0, inf to c1).  The query -1.4e19 e_H probes list 1 then list 0 with finite coarse values and scores (2.8e19)^2 = +inf against the
two rows inside the scan; +1.4e19 e_H has one finite probe and one -1; the NaN, inf, 1e30 and 1.5e19 queries have no finite coarse value at all."""
import functools

import numpy as np

import nonfinite_cases as nfc
from admission_rule import admitted  # noqa: F401  (re-exported for the two test modules)
from nonfinite_cases import classes, id_map  # noqa: F401
from oracle import oracle as orc

L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
FLT_MAX = np.float32(np.finfo(np.float32).max)
N = 20000 + 77
DIMS = (20, 100, 160)
H, NAN_COL = 5, 2
NQ, K = 24, 10
BOUNDARY = 5120
CONTROLS, COPIES = (0, 6, 23), (6, 23)
Q_NAN_POS, Q_INF_NEG, Q_NAN_NEG, Q_INF_POS, Q_ZERO, Q_POS, Q_NEG, Q_1E30, Q_SQUARES = 1, 2, 3, 4, 5, 7, 8, 9, 10
HOSTILE_QUERIES = (Q_NAN_POS, Q_INF_NEG, Q_NAN_NEG, Q_INF_POS, Q_ZERO, Q_POS, Q_NEG, Q_1E30, Q_SQUARES)
PLANTED = (10, BOUNDARY - 20, BOUNDARY + 10, 12000, N - 40)  # case "finite": the only rows with a positive H
HOSTILE_KINDS = ("nan+", "nan-", "inf+", "inf-", "1e30", "1.5e19", "tiny")
CASES = ("finite", "hostile")


def neutral(metric):
    return FLT_MAX if metric == L2 else -FLT_MAX


def bn(d):
    """rows per tile of flat_mfma_kernel: the resident geometry up to d = 128, the wide one beyond"""
    return 64 if d <= 128 else 256


def split_rows(n, d, nsplit):
    """rows per split of flat_mfma_kernel's plan (csrc/flat_mfma.hip plan_flat_mfma) for the split count it reports"""
    ntiles = -(-n // bn(d))
    return -(-ntiles // nsplit) * bn(d)


def hostile_rows(n=N, boundary=BOUNDARY):
    """kind -> its three rows: before the boundary, after it, in the last partial tile"""
    return {kind: (boundary - 1 - i, boundary + i, n - 1 - i) for i, kind in enumerate(HOSTILE_KINDS)}


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _ordinary_rows(rng, n, d):
    xb = rng.standard_normal((n, d)).astype(np.float32)
    col = (-np.abs(rng.standard_normal(n)) - 0.25).astype(np.float32)
    col[rng.random(n) < 0.3] = 0.0
    xb[:, H] = col
    return xb


def _make_hostile(xb, where):
    bits = xb.view(np.uint32)
    for kind, rows in where.items():
        for r in rows:
            if kind == "nan+":
                bits[r, NAN_COL] = 0x7FC00000
            elif kind == "nan-":
                bits[r, NAN_COL] = 0xFFC00000
            elif kind == "inf+":
                xb[r, H] = np.inf
            elif kind == "inf-":
                xb[r, H] = -np.inf
            elif kind == "1e30":
                xb[r] = 1e30
            elif kind == "1.5e19":
                xb[r] = 1.5e19
            else:
                xb[r] *= np.float32(1e-20)


def queries(d, rng, nq=NQ):
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    bits = xq.view(np.uint32)
    bits[Q_NAN_POS, H] = 0x7FC00000
    bits[Q_NAN_NEG, H] = 0xFFC00000  # (through the integer view: arithmetic would be free to change the sign)
    xq[Q_INF_NEG, H] = -np.inf
    xq[Q_INF_POS, H] = np.inf
    xq[Q_ZERO, H] = 0.0
    xq[Q_POS, H] = 2.0
    xq[Q_NEG, H] = -2.0
    xq[Q_1E30] = 1e30
    xq[Q_SQUARES] = 1.5e19
    for c in COPIES:
        xq[c] = xq[0]
    return xq


@functools.lru_cache(maxsize=None)
def flat_inputs(case, d):
    """-> dict(xb, xq, ids, planted, hostile), read-only arrays built once"""
    assert case in CASES and d in DIMS
    rng = np.random.default_rng(1000 + d)  # (both cases of a dimension share their ordinary rows and their queries)
    xb = _ordinary_rows(rng, N, d)
    xq = queries(d, rng)
    if case == "finite":
        planted, where = PLANTED, {}
        xb[list(PLANTED), H] = [0.5, 1.0, 2.0, 0.75, 1.5]
    else:
        where = hostile_rows()
        _make_hostile(xb, where)
        planted = tuple(sorted(r for kind in ("inf+", "1e30", "1.5e19") for r in where[kind]))  # the rows with a positive H
    return _freeze(dict(xb=xb, xq=xq, ids=id_map(N), planted=planted, hostile=where))


def keep_rows(case, d):
    """the rows an IDSelectorBatch of the selector cases keeps: about 40 %, every second hostile row and every second planted row among them"""
    c = flat_inputs(case, d)
    keep = np.random.default_rng(7).random(N) < 0.4
    special = sorted({r for rows in c["hostile"].values() for r in rows} | set(c["planted"]))
    keep[special] = np.arange(len(special)) % 2 == 0
    return np.flatnonzero(keep).astype(np.int64)


def flat_path(nq, sel=None):
    return orc.PATH_AUTO if sel is not None else (orc.PATH_BLAS if nq >= 20 else orc.PATH_PAIR)


def expected(case, metric, k, nq, d=20, idmap=False, sel=None):
    """the oracle's own Flat search of the batch's first nq queries: the BLAS branch from 20 queries on, the per-pair branch below (and
    whatever its own dispatch says with a selector); idmap: labels through id_map"""
    c = flat_inputs(case, d)
    with np.errstate(all="ignore"):
        return orc.flat_search(metric, c["xb"], c["xq"][:nq], k, force_path=flat_path(nq, sel), sel=sel, id_map=c["ids"] if idmap else None)


@functools.lru_cache(maxsize=None)
def flat_scores(case, d, metric, branch):
    """[NQ, N] f32 scores of one branch, no heap.  "pair": the per-pair chains.  "blas": (xn + yn) - 2 ip in f32 from the oracle's norms and
    its inner-product chains (FAISS clamps a negative value to 0: a comparison, which leaves a NaN alone); inner product has one branch"""
    c = flat_inputs(case, d)
    with np.errstate(all="ignore"):
        if metric == IP or branch == "pair":
            out = orc.pair_chains(metric, c["xb"], c["xq"])
        else:
            ip = orc.pair_chains(IP, c["xb"], c["xq"])
            xn, yn = orc.norms(c["xq"]), orc.norms(c["xb"])
            out = (xn[:, None] + yn[None, :]) - np.float32(2) * ip
            out = np.where(out < 0, np.float32(0), out).astype(np.float32)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------------------ IVF2,Flat
N_IVF = 3000
IVF_DIMS = (20, 128)
IVF_EARLY, IVF_LATE = 40, N_IVF - 400  # hostile rows start here: among the first 256 arrivals of their list, and behind them
Q_NO_COARSE, Q_FAR, Q_ONE_PROBE = 24, 25, 26  # (IVF batches: 27 queries)
NQ_IVF = 27
IVF_PLANTED_L2 = (IVF_EARLY + 20, IVF_LATE + 20)


def _ivf_hostile_rows():
    return {kind: (IVF_EARLY + i, IVF_LATE + i) for i, kind in enumerate(HOSTILE_KINDS)}


@functools.lru_cache(maxsize=None)
def ivf_inputs(metric, d):
    """-> dict(xb, xq, ids, cent, hostile, planted)"""
    assert d in IVF_DIMS
    rng = np.random.default_rng(2000 + d + metric)
    xq = np.concatenate([queries(d, rng), rng.standard_normal((NQ_IVF - NQ, d)).astype(np.float32)])
    xq[Q_NO_COARSE, 0::2] = np.inf
    xq[Q_NO_COARSE, 1::2] = -np.inf
    if metric == IP:
        cent = nfc.centroids(d)
        xb = _ordinary_rows(rng, N_IVF, d)
        xb[:, 0] += np.where(rng.random(N_IVF) < 0.5, 4.0, -1.5).astype(np.float32)  # (H's mean is negative: keep both lists long)
        where = _ivf_hostile_rows()
        _make_hostile(xb, where)
        planted = (IVF_EARLY + 30, IVF_LATE + 30)
        xb[list(planted)] = np.abs(xb[list(planted)])  # <x, c0> positive: list 0, with a positive H
        xb[list(planted), H] = [1.0, 2.0]
        xq[Q_FAR, 9] = 3e38  # the coarse values are finite (+-1.5e38), the fine scores overflow to +-inf for every component beyond +-1.13
        xq[Q_ONE_PROBE] = xq[Q_INF_POS]  # coarse values +inf and -inf: one probe and one -1
    else:
        cent = np.zeros((2, d), dtype=np.float32)
        cent[1, H] = -1e19
        xb = rng.standard_normal((N_IVF, d)).astype(np.float32)
        far = rng.random(N_IVF) < 0.5
        xb[far, H] = (np.float32(-1e19) + rng.random(int(far.sum())).astype(np.float32) * np.float32(1e18)).astype(np.float32)
        where = {kind: rows for kind, rows in _ivf_hostile_rows().items() if kind.startswith("nan")}
        _make_hostile(xb, where)
        planted = IVF_PLANTED_L2
        for p in planted:
            xb[p] = 0.0
            xb[p, H] = 1.4e19
        for q in (7, 8, 11, 12):  # finite queries near c1 (the others are near c0)
            xq[q, H] = np.float32(-1e19) + np.float32(q * 6e16)
        xq[Q_FAR] = 0.0
        xq[Q_FAR, H] = -1.4e19
        xq[Q_ONE_PROBE] = 0.0
        xq[Q_ONE_PROBE, H] = 1.4e19
    return _freeze(dict(xb=xb, xq=xq, ids=id_map(N_IVF), cent=cent, hostile=where, planted=planted))


@functools.lru_cache(maxsize=None)
def ivf_oracle(metric, d, idmap=False):
    """the oracle's IVF2,Flat (or IDMap,IVF2,Flat) over ivf_inputs, built once; search only"""
    c = ivf_inputs(metric, d)
    o = orc.Index(d, ("IDMap," if idmap else "") + "IVF2,Flat", metric)
    o.ivf_set_centroids(c["cent"])
    with np.errstate(all="ignore"):
        if idmap:
            o.add_with_ids(c["xb"], c["ids"])
        else:
            o.add(c["xb"])
    return o


def ivf_expected(metric, d, k, nprobe, idmap=False, nq=NQ_IVF):
    return ivf_oracle(metric, d, idmap).search(ivf_inputs(metric, d)["xq"][:nq], k, nprobe=nprobe)


def ivf_probes(metric, d, nprobe=2):
    """[NQ_IVF, nprobe] the probed lists in rank order, -1 where the quantiser's heap admitted none"""
    c = ivf_inputs(metric, d)
    return orc.flat_search(metric, c["cent"], c["xq"], nprobe)[1]


def ivf_range(metric, d, radius, nprobe, idmap=False):
    """(lims, D, I) of a range search over ivf_inputs: per query the rows of its probed lists whose per-pair chain passes, in (probe rank,
    position) order -- range_reference.ivf_range fed from the raw chains, which are defined for a NaN too"""
    import range_reference as rr

    c, o = ivf_inputs(metric, d), ivf_oracle(metric, d)
    lists = [o.ivf_list(l) for l in range(2)]
    with np.errstate(all="ignore"):
        dis = [orc.pair_chains(metric, rows, c["xq"]) for _, rows in lists]
    P = ivf_probes(metric, d, nprobe)
    lims, D, I = np.zeros(NQ_IVF + 1, dtype=np.int64), [np.empty(0, dtype=np.float32)], [np.empty(0, dtype=np.int64)]
    for q in range(NQ_IVF):
        cnt = 0
        for l in P[q]:
            if l < 0:
                continue
            h = rr.hits(metric, dis[l][q], radius)
            D.append(dis[l][q][h])
            I.append(c["ids"][lists[l][0][h]] if idmap else lists[l][0][h])
            cnt += int(h.sum())
        lims[q + 1] = lims[q] + cnt
    return lims, np.concatenate(D), np.concatenate(I)


# ------------------------------------------------------------------------------- IVF<n>,Flat at d = 128 on the bf16 coarse filter
FILTER_D, FILTER_NQ, FILTER_HOSTILE = 128, 40, 8  # queries 0 ... 7 have H exactly 0 and probe the planted rows' list first
FILTER_Q_NAN, FILTER_Q_BIG = 8, 9


@functools.lru_cache(maxsize=None)
def _filter_base(metric, nlist, n):
    xb = orc.synth_clustered(n, FILTER_D, 5, n_centers=nlist, sigma=0.2)
    o = orc.Index(FILTER_D, f"IVF{nlist},Flat", metric)
    o.train(xb)
    return _freeze(dict(xb=xb, cent=o.ivf_centroids()))


@functools.lru_cache(maxsize=None)
def filter_inputs(metric, nlist, n, m):
    """the shapes the suite uses for the bf16 coarse filter, trained centroids.  Under inner product rows 0 ... m - 1 hold +inf in H: they
    are the first m arrivals of one list, `planted_list`.  Queries 0 ... FILTER_HOSTILE - 1 are later rows of that list with H set to exactly 0
    (chosen among those that probe it first): the planted rows score 0 * inf = NaN against them.  Query 8 holds a NaN, query 9 is times 1e19.
    -> dict(xb, xq, cent, oracle, planted_list)"""
    b = _filter_base(metric, nlist, n)
    xb = b["xb"].copy()
    assert m == 0 or metric == IP  # (under L2 a row with an inf has no finite coarse value and is stored nowhere)
    xb[:m, H] = np.inf
    o = orc.Index(FILTER_D, f"IVF{nlist},Flat", metric)
    o.ivf_set_centroids(b["cent"])
    with np.errstate(all="ignore"):
        o.add(xb)
    xq = orc.synth_clustered(FILTER_NQ, FILTER_D, 6, n_centers=nlist, sigma=0.2)
    star = -1
    if m:
        star = next(l for l in range(nlist) if 0 in o.ivf_list(l)[0][:1])
        ids = o.ivf_list(star)[0]
        assert ids[:m].tolist() == list(range(m))
        cand = xb[ids[m:256]].copy()
        cand[:, H] = 0.0
        first = orc.flat_search(metric, b["cent"], np.concatenate([cand, cand[: max(0, 20 - len(cand))]]), 1)[1][: len(cand), 0]
        cand = cand[first == star]
        assert len(cand) >= FILTER_HOSTILE
        xq[:FILTER_HOSTILE] = cand[:FILTER_HOSTILE]
    xq.view(np.uint32)[FILTER_Q_NAN, 7] = 0x7FC00000
    xq[FILTER_Q_BIG] *= np.float32(1e19)
    return _freeze(dict(xb=xb, xq=xq, cent=b["cent"], oracle=o, planted_list=star))
