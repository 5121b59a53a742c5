"""The non-finite search cases of the scanning coded kinds and their CPU answers: inputs and models of tests/test_coded_nonfinite_gpu.py,
whose preconditions tests/test_admission_rule_cpu.py asserts without a GPU.  A helper module: nothing here is collected.

Rows, codebooks, ranges and centroids are finite, ordinary values; only queries are hostile.  The batch (component H = HOSTILE):

  q0, q7, q16   finite controls; q7 and q16 are copies of q0 (q7 shares its interleaved group with q4 ... q6, q16 sits in the last, partial one)
  q1            component H = NaN 0x7FC00000          q2   component H = NaN 0xFFC00000
  q3            component H = +inf                     q4   component H = -inf
  q5            every component 1e30                   q6   every component 1.5e19 (a square is finite, two of them are not)
  the others    finite
  q17 (IVF)     +inf / -inf alternating: no finite coarse value under either metric, every probe is -1
  q18 (IVF)     component BIG = 3e38: under inner product the coarse values are finite (+-1.5e38) and every fine score is +-inf

What the parameters hold in column H so that an inner product with q3 / q4 has rows scoring +inf, -inf and NaN:
  PQ     the codebook of H's sub-space has entries 0 ... 2 with a POSITIVE value in column H, entries 3 ... 39 with exactly 0, the others
         negative.  Entries 0 ... 2 lie far from ordinary rows, so only the PLANTED rows carry their codes: q3 has len(PLANTED) admissible rows
         (between 1 and k - 1 at k = 10, on both sides of position 8192), q4 has thousands
  SQ8    a[H] = -100, s[H] = 2: code 49 decodes to -2, code 50 to exactly 0, code 51 to 2; the rows' values of H are -2 or 0 (+ noise inside
         the code's bin), the planted rows' 2
  IVF    centroid 1 = -centroid 0 = -0.5 everywhere: q3's base <x, c> is +inf for list 0 and -inf for list 1, so q3 probes list 0 alone and
         its rows score +inf (planted) or NaN; q4 probes list 1 alone, whose rows score +inf or NaN
Under L2 every hostile query has no admissible row at all (with ordinary rows an L2 sum is either finite for every row or for none).  For
the IVF kinds that happens at the quantiser: every hostile L2 query, q18 included, has no finite coarse value, is probed nowhere and
reaches no scan kernel -- the IVF L2 cases pin the -1-probe path only (DESIGN.md 5 says what a case that reaches the scan needs)."""
import functools

import numpy as np

import ivfpq_reference as ivr
import pq_reference as pqr
import sq_reference as sqr
from admission_rule import admitted
from oracle import oracle as orc

L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
R = 8192  # rows / positions per scan workgroup = entries of a bucket (the GPU test asserts the statistic equals it)
N_FLAT = 2 * R + 77
N_IVF = 20000
NQ = 17
KS = (1, 10)
HOSTILE, BIG = 5, 9
CONTROLS, COPIES = (0, 7, 16), (7, 16)
Q_NAN_POS, Q_NAN_NEG, Q_INF_POS, Q_INF_NEG, Q_1E30, Q_SQUARES, Q_NO_COARSE, Q_FINE_BEYOND = 1, 2, 3, 4, 5, 6, 17, 18
PLANTED_FLAT = (10, 4000, 9000, 12000, N_FLAT - 1)
PLANTED_IVF = (10, 5000, 17500, 18500, N_IVF - 1)  # all sent to list 0, which takes about every second row: positions ~5 ... ~10000

# kind -> family, d, M; the IDMap variants share the data of their base kind
KINDS = {
    "PQ8": ("pq", 32, 8),  # float4 table entries, query block 16
    "PQ80": ("pq", 160, 80),  # scalar entries, query block 1
    "SQ8": ("sq", 20, 0),
    "IVF2,PQ8": ("ivfpq", 32, 8),
    "IVF2,SQ8": ("ivfsq", 20, 0),
}
IDMAP_KINDS = ("IDMap,PQ8", "IDMap,IVF2,SQ8")


def base_kind(kind):
    return kind[len("IDMap,") :] if kind.startswith("IDMap,") else kind


def id_map(n):
    return np.arange(n, dtype=np.int64) * 7 + 1000003  # (no id is a row number)


def queries(d, rng, ivf, col=HOSTILE):
    xq = rng.standard_normal((NQ + (2 if ivf else 0), d)).astype(np.float32)
    bits = xq.view(np.uint32)
    bits[Q_NAN_POS, col] = 0x7FC00000
    bits[Q_NAN_NEG, col] = 0xFFC00000  # (through the integer view: arithmetic would be free to change the sign)
    xq[Q_INF_POS, col] = np.inf
    xq[Q_INF_NEG, col] = -np.inf
    xq[Q_1E30] = 1e30
    xq[Q_SQUARES] = 1.5e19
    for c in COPIES:
        xq[c] = xq[0]
    if ivf:
        xq[Q_NO_COARSE, 0::2] = np.inf
        xq[Q_NO_COARSE, 1::2] = -np.inf
        xq[Q_FINE_BEYOND, BIG] = 3e38
    return xq


def hostile_column(rng, n=pqr.KSUB):
    """values of column H over a codebook's entries: 0 ... 2 positive, 3 ... 39 exactly zero, the others negative"""
    col = (-np.abs(rng.standard_normal(n)) - 0.25).astype(np.float32)
    col[3:40] = 0.0
    col[:3] = [0.5, 1.0, 2.0]
    return col


def codebooks(rng, M, dsub):
    cb = pqr.synthetic_codebooks(rng, M, dsub)
    m, j = divmod(HOSTILE, dsub)
    cb[m, :, j] = hostile_column(rng)
    cb[m, :3, (j + 1) % dsub] = [6.0, 7.0, 8.0]  # entries 0 ... 2: far from every ordinary row
    mb, jb = divmod(BIG, dsub)
    cb[mb, :, jb] = np.where(cb[mb, :, jb] < 0, -2.0, 2.0) + cb[mb, :, jb]  # |value| >= 2: 3e38 times it overflows
    return cb


def sq_range(d):
    """(vmin, vdiff): ordinary components cover [-5, 5]; H decodes to -100 + 2 code; BIG to [2, 6]"""
    vmin, vdiff = np.full(d, -5.0, dtype=np.float32), np.full(d, 10.0, dtype=np.float32)
    vmin[HOSTILE], vdiff[HOSTILE] = -101.0, 510.0
    vmin[BIG], vdiff[BIG] = 2.0, 4.0
    return vmin, vdiff


def centroids(d):
    c = np.full((2, d), 0.5, dtype=np.float32)
    c[1] = -c[0]
    return c


@functools.lru_cache(maxsize=None)
def inputs(kind):
    """-> dict(d, M, family, xb, xq, ids, and the kind's parameters), read-only arrays, built once per base kind"""
    family, d, M = KINDS[kind]
    ivf = family.startswith("ivf")
    rng = np.random.default_rng(sum(map(ord, kind)))
    n = N_IVF if ivf else N_FLAT
    planted = PLANTED_IVF if ivf else PLANTED_FLAT
    xb = rng.standard_normal((n, d)).astype(np.float32)
    out = dict(family=family, d=d, M=M, ivf=ivf, planted=planted)
    if ivf:
        out["cent"] = centroids(d)
        xb[list(planted)] += 1.0  # <x, c0> clearly positive: list 0 under both metrics
    cl = out["cent"][0] if ivf else np.zeros(d, dtype=np.float32)
    if family.endswith("pq"):
        dsub = d // M
        cb = out["cb"] = codebooks(rng, M, dsub)
        m = HOSTILE // dsub
        for i, p in enumerate(planted):  # (residual) sub-vector m = entry i % 3
            xb[p, m * dsub : (m + 1) * dsub] = cl[m * dsub : (m + 1) * dsub] + cb[m, i % 3]
    else:
        out["vmin"], out["vdiff"] = sq_range(d)
        centre = np.where(rng.random(n) < 0.7, -2.0, 0.0)
        centre[list(planted)] = 2.0
        xb[:, HOSTILE] = centre + rng.uniform(-0.3, 0.3, n)  # (the residual moves it by 0.5 more: inside the code's bin of +-1)
        if ivf:
            xb[:, 0] += 1.4  # (H's mean is -1.4: without this list 0 would take a third of the rows and stay below R)
    out["xb"], out["xq"], out["ids"] = xb, queries(d, rng, ivf), id_map(n)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scores(kind, metric):
    """the model's scores of every query, computed once per (base kind, metric).  Flat kinds: dis [nq, n].  IVF kinds: (P [nq, 2] probed lists in
    rank order, lists, dis per list [nq, n_l])"""
    c = inputs(kind)
    with np.errstate(all="ignore"):
        if c["family"] == "pq":
            return pqr.distances(pqr.tables(c["cb"], c["xq"], metric), pqr.encode(c["cb"], c["xb"]))
        if c["family"] == "sq":
            return sqr.sq_distances(metric, c["vmin"], c["vdiff"], sqr.encode(c["vmin"], c["vdiff"], c["xb"]), c["xq"])
        if c["family"] == "ivfpq":
            lists = ivr.build_lists(metric, c["cent"], c["cb"], c["xb"])
            return ivr.probes(metric, c["cent"], c["xq"], 2), lists, ivr.all_pair_distances(metric, c["cent"], c["cb"], lists, c["xq"])
        lists = sqr.build_lists(metric, c["cent"], c["vmin"], c["vdiff"], c["xb"])
        return (sqr.probes(metric, c["cent"], c["xq"], 2), lists,
                sqr.all_pair_distances(metric, c["cent"], c["vmin"], c["vdiff"], lists, c["xq"]))  # fmt: skip


def expected(kind, metric, k):
    """(D, I) of the whole batch; kind may be an IDMap variant"""
    base = base_kind(kind)
    c, s = inputs(base), scores(base, metric)
    labels = c["ids"] if kind != base else None
    with np.errstate(all="ignore"):
        if c["family"] == "pq":
            return pqr.select(s, k, metric, labels=labels)
        if c["family"] == "sq":
            return sqr.sq_select(s, k, metric, labels=labels)
        P, lists, dl = s
        return (ivr.select if c["family"] == "ivfpq" else sqr.ivf_select)(metric, P, lists, dl, k, id_map=labels)


def score_rows(kind, metric):
    """per query (scores [n_q] f32, positions [n_q]) of the rows it scans: every row (flat kinds) or the rows of its probed lists with their
    positions in the list (IVF kinds)"""
    c, s = inputs(kind), scores(kind, metric)
    if not c["ivf"]:
        return [(s[q], np.arange(s.shape[1])) for q in range(s.shape[0])]
    P, lists, dl = s
    out = []
    for q in range(P.shape[0]):
        ls = [l for l in P[q] if l >= 0 and lists[l][0].size]
        out.append((np.concatenate([dl[l][q] for l in ls]) if ls else np.empty(0, dtype=np.float32),
                    np.concatenate([np.arange(lists[l][0].size) for l in ls]) if ls else np.empty(0, dtype=np.int64)))  # fmt: skip
    return out


def classes(v):
    """the classes present in a score array"""
    v = np.asarray(v, dtype=np.float32)
    out = set()
    if np.isnan(v).any():
        out.add("nan")
    if (v == np.inf).any():
        out.add("+inf")
    if (v == -np.inf).any():
        out.add("-inf")
    if np.isfinite(v).any():
        out.add("finite")
    return out


# what each hostile query's score row must hold, by family group and metric (the docstring above says why)
EXPECTED_CLASSES = {
    ("flat", L2): {Q_NAN_POS: {"nan"}, Q_NAN_NEG: {"nan"}, Q_INF_POS: {"+inf"}, Q_INF_NEG: {"+inf"}, Q_1E30: {"+inf"}, Q_SQUARES: {"+inf"}},
    ("flat", IP): {Q_NAN_POS: {"nan"}, Q_NAN_NEG: {"nan"}, Q_INF_POS: {"+inf", "-inf", "nan"}, Q_INF_NEG: {"+inf", "-inf", "nan"},
                   Q_1E30: {"finite"}, Q_SQUARES: {"finite"}},  # fmt: skip
    # (an L2 query without a finite coarse value scans nothing)
    ("ivf", L2): {Q_NAN_POS: set(), Q_NAN_NEG: set(), Q_INF_POS: set(), Q_INF_NEG: set(), Q_1E30: set(), Q_SQUARES: set(), Q_NO_COARSE: set(),
                  Q_FINE_BEYOND: set()},  # fmt: skip
    ("ivf", IP): {Q_NAN_POS: set(), Q_NAN_NEG: set(), Q_INF_POS: {"+inf", "nan"}, Q_INF_NEG: {"+inf", "nan"}, Q_1E30: {"finite"},
                  Q_SQUARES: {"finite"}, Q_NO_COARSE: set()},  # fmt: skip
}


# ------------------------------------------------------------------------------------------------ best-last rows: bucket overflow
N_OVERFLOW = {"PQ8": 3 * R + 5, "PQ80": 3 * R + 5, "SQ8": 2 * R + 5}


@functools.lru_cache(maxsize=None)
def overflow_inputs(kind, metric):
    """the hostile batch against rows whose scores IMPROVE with the row number for the control queries, so that whole ranges beat the bound and
    the buckets overflow.  The rows exist as codes only (written through an index file): components 0 and 1 (PQ: the first component of
    sub-spaces 0 and 1) spell the row number v as (256 (v // 256), v % 256); the hostile component is the LAST one.
    -> dict(d, M, codes, xq, col, and the parameters)"""
    family, d, M = KINDS[kind]
    n = N_OVERFLOW[kind]
    assert n <= 65536
    rng = np.random.default_rng(sum(map(ord, kind)) + 17)
    col = d - 1
    xq = queries(d, rng, False, col)
    v = np.arange(n)
    out = dict(family=family, d=d, M=M, n=n, col=col)
    if family == "pq":
        dsub = d // M
        cb = pqr.synthetic_codebooks(rng, M, dsub)
        cb[:2] = 0.0
        cb[0, :, 0] = 256.0 * np.arange(256)
        cb[1, :, 0] = np.arange(256)
        cb[M - 1, :, dsub - 1] = hostile_column(rng)
        codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
        codes[:, 0], codes[:, 1] = v // 256, v % 256
        c0, c1 = 0, dsub
        out["cb"] = cb
    else:
        vmin, vdiff = sq_range(d)
        vmin[HOSTILE], vdiff[HOSTILE] = vmin[0], vdiff[0]  # (the hostile component is the last one here)
        vmin[col], vdiff[col] = -101.0, 510.0
        vmin[:2], vdiff[:2] = [-128.0, -0.5], [256.0 * 255.0, 255.0]  # s = (256, 1), a = 0: codes (c0, c1) decode to (256 c0, c1)
        codes = rng.integers(0, 256, (n, d)).astype(np.uint8)
        codes[:, 0], codes[:, 1] = v // 256, v % 256
        codes[:, col] = rng.choice(np.array([49, 50, 51], dtype=np.uint8), n, p=[0.6, 0.3, 0.1])
        c0, c1 = 0, 1
        out["vmin"], out["vdiff"] = vmin, vdiff
    for q in CONTROLS:  # L2: far beyond the last row; inner product: the score is the row number
        xq[q, c0], xq[q, c1] = (256.0 * 300, 300.0) if metric == L2 else (1.0, 1.0)
    out["codes"], out["xq"] = codes, xq
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def overflow_scores(kind, metric):
    c = overflow_inputs(kind, metric)
    with np.errstate(all="ignore"):
        if c["family"] == "pq":
            return pqr.distances(pqr.tables(c["cb"], c["xq"], metric), c["codes"])
        return sqr.sq_distances(metric, c["vmin"], c["vdiff"], c["codes"], c["xq"])


def overflow_expected(kind, metric, k):
    c, s = overflow_inputs(kind, metric), overflow_scores(kind, metric)
    with np.errstate(all="ignore"):
        return pqr.select(s, k, metric) if c["family"] == "pq" else sqr.sq_select(s, k, metric)
