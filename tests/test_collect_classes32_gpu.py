"""The int8 store's 32 row classes for k <= 16 (csrc/flat_collect.hip collect_slot_stride, the 32-class register pre-pass and the paced
bound upkeep; DESIGN.md 3.1 "row classes"): on the smallest int8 store with a ragged end the coarse filter returns the exact f32 kernel's
labels and distance bits for k = 1, 10, 16, L2 and inner product, a batch with one partial query block and one of two blocks, with an
IDSelector and at d = 40; rows planted so that the nearest ones share a class, sit 16 rows apart, fill sixteen classes, or lie in the
pre-pass's rows and in the store's last stage do not disturb it; and 32 classes leave fewer candidates than 16.  The slot rule itself
takes 32 classes from k = 15 on (below that the 32-class scan measured slower): every case runs with 32 classes asked for through the
option cl_classes, and once more as the rule decides."""

import numpy as np
import pytest

L2, IP = 1, 0
KERNEL = "flat_bf16_collect_kernel"
NB = 262144 + 77  # the smallest store that gets int8 rows, and a last stage of 77 rows
NQ = 600          # 512 + 88: a full query block and one of three tile columns; [:130]: one block of five columns, beyond the small-batch path


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss

    return mi355_faiss


def _index(mf, d, metric, xb, prefilter):
    ix = mf.index_factory(d, "Flat", metric)
    ix.set_option("prefilter", prefilter)
    for i0 in range(0, len(xb), 1 << 16):
        ix.add(xb[i0 : i0 + (1 << 16)])
    return ix


def _same(a, b):
    (D1, I1), (D2, I2) = a, b
    return np.array_equal(I1, I2) and np.array_equal(D1.view(np.uint32), D2.view(np.uint32))


@pytest.fixture(scope="module")
def data():
    rs = np.random.RandomState(3232)
    return rs.rand(NB, 128).astype(np.float32), rs.rand(NQ, 128).astype(np.float32)


@pytest.fixture(scope="module")
def pair(mf, data):
    """per metric: the coarse-filter index and the exact one over the same rows, built once"""
    made = {}

    def get(metric):
        if metric not in made:
            made[metric] = (_index(mf, 128, metric, data[0], 2), _index(mf, 128, metric, data[0], 0))
        return made[metric]

    return get


def _check(cl, ex, xq, k, sel=None):
    """one search on 32 classes against the exact kernel, one as the slot rule decides, then the same index on the bf16 store: 16
    classes, the same lists"""
    kw = {} if sel is None else {"sel": sel}
    ref = ex.search(xq, k, **kw)
    ovf = cl.collect_stats()["overflows"]
    cl.set_option("cl_classes", 32)
    try:
        got = cl.search(xq, k, **kw)
        assert cl.last_kernel_info()["name"] == KERNEL
        assert _same(got, ref), "32 row classes: labels or distance bits differ from the exact kernel"
        assert cl.collect_stats()["overflows"] == ovf
        assert cl.get_stat("cl_store_i8") == 1
        assert cl.get_stat("cl_row_classes") == 32
        cl.set_option("cl_classes", 0)
        assert _same(cl.search(xq, k, **kw), ref), "the rule's classes: labels or distance bits differ from the exact kernel"
        assert cl.get_stat("cl_row_classes") == (32 if k >= 15 else 16) and cl.get_stat("cl_store_i8") == 1
        assert cl.collect_stats()["overflows"] == ovf
        cl.set_option("cl_i8", 0)
        assert _same(cl.search(xq, k, **kw), ref), "bf16 store: labels or distance bits differ from the exact kernel"
        assert cl.get_stat("cl_row_classes") == 16 and cl.get_stat("cl_store_i8") == 0
    finally:
        cl.set_option("cl_classes", 0)
        cl.set_option("cl_i8", 1)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [130, NQ])
@pytest.mark.parametrize("k", [1, 10, 16])
def test_classes32_equal_the_exact_kernel(pair, data, metric, nq, k):
    cl, ex = pair(metric)
    _check(cl, ex, data[1][:nq], k)


@pytest.mark.gpu
def test_classes32_with_selector(pair, data):
    cl, ex = pair(L2)
    _check(cl, ex, data[1], 10, sel=("batch", np.arange(1, NB, 3, dtype=np.int64)))


@pytest.mark.gpu
def test_classes32_d40(mf):
    rs = np.random.RandomState(40)
    xb = rs.rand(NB, 40).astype(np.float32)
    xq = rs.rand(130, 40).astype(np.float32)
    _check(_index(mf, 40, L2, xb, 2), _index(mf, 40, L2, xb, 0), xq, 10)


# Planted rows.  Scenario s of batch b plants for three queries -- in the first, a middle and the last live tile column of the batch --
# rows that beat every natural row and stay inside the data's range (the store must remain an int8 one): L2: the query plus a step that
# grows with the rank; inner product: the query's components pushed to the end of the range on their side of the middle (48 against the
# 43 of the best natural row, 32 with any other query).
# (a) ten rows of ONE class mod 32: the bound has to come from the other classes' natural rows and must not cut the ten off
# (b) two rows 16 apart: one class of 16, two of 32
# (c) sixteen rows in sixteen classes mod 32 that are eight classes mod 16, for k = 16: every class slot that counts holds a planted row
# (d) a row inside the pre-pass's first 32 768 rows and one in the store's last, ragged stage
SCEN_K = {"a": 10, "b": 10, "c": 16, "d": 10}
# the queries of scenario number si: nq = 130 (five live columns; the last holds queries 128 and 129: (a) and (b) get them, (c) and (d) the
# column before it), nq = 600 (block 0: columns 0 and 9; block 1: the last of its three live columns)
def _queries(nq, si):
    return (si, 66 + si, (128, 129, 126, 127)[si]) if nq == 130 else (4 + si, 290 + si, 592 + si)


def _plant_rows(scen, j):
    """rows of scenario `scen` for its j-th planted query (j = 0 .. 5 over both batches): disjoint between scenarios and queries"""
    base = 32 * (1000 + 700 * j)
    if scen == "a":
        return [base + 7 + 32 * 41 * m for m in range(10)]
    if scen == "b":
        return [base + 32 * 300 + 9, base + 32 * 300 + 25]
    if scen == "c":
        cls = list(range(8)) + list(range(16, 24))
        return [base + 32 * (400 + 11 * m) + cls[m] for m in range(16)]
    return [2000 + 64 * j + 3, NB - 70 + 11 * j]


@pytest.fixture(scope="module")
def planted(mf, data):
    made = {}

    def get(metric):
        if metric in made:
            return made[metric]
        xb, xq = data[0].copy(), data[1]
        rs = np.random.RandomState(99)
        step = rs.rand(128).astype(np.float32) - 0.5
        rows = {}
        for si, scen in enumerate("abcd"):
            j = 0
            for nq in (130, NQ):
                for q in _queries(nq, si):
                    rr = _plant_rows(scen, j)
                    for m, r in enumerate(rr):
                        if metric == L2:
                            xb[r] = np.clip(xq[q] + np.float32(0.02 * (m + 1)) * step, 0.0, 1.0)
                        else:
                            xb[r] = np.clip(0.5 + np.float32(40 - 2 * m) * (xq[q] - 0.5), 0.02, 0.98)
                    rows[(scen, nq, q)] = rr
                    j += 1
        flat = [r for rr in rows.values() for r in rr]
        assert len(set(flat)) == len(flat) and max(flat) < NB
        made[metric] = (_index(mf, 128, metric, xb, 2), _index(mf, 128, metric, xb, 0), rows)
        return made[metric]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [130, NQ])
@pytest.mark.parametrize("k", [10, 16])
def test_classes32_planted_rows(planted, data, metric, nq, k):
    cl, ex, rows = planted(metric)
    _, I = _check(cl, ex, data[1][:nq], k)
    seen = 0
    for (scen, n, q), rr in rows.items():
        if n != nq or SCEN_K[scen] != k:
            continue
        assert set(I[q][: len(rr)].tolist()) == set(rr), (scen, q, I[q].tolist(), rr)  # the planted rows are the nearest
        seen += 1
    assert seen == (9 if k == 10 else 3)
    for scen in "abcd":  # what the scenarios claim about classes
        rr = _plant_rows(scen, 0)
        c32, c16 = {r & 31 for r in rr}, {r & 15 for r in rr}
        assert {"a": len(c32) == 1, "b": len(c32) == 2 and len(c16) == 1, "c": len(c32) == 16 and len(c16) == 8,
                "d": rr[0] < 32768 and rr[1] >= NB - 77}[scen]


@pytest.mark.gpu
def test_classes32_leave_fewer_candidates_than_16(pair, data):
    """uniform rows, k = 10, nq = 600: candidates per query that reach the exact stage, the same index on 32 and on 16 classes
    (option cl_classes).  Measured on MI355X: 29.0 per query on 32 classes, 36.4 on 16 (profiles/scan_classes_ab.txt)."""
    cl, ex = pair(L2)

    def per_query(opt):
        cl.set_option("cl_classes", opt)
        c0 = cl.collect_stats()
        got = cl.search(data[1], 10)
        c1 = cl.collect_stats()
        assert c1["overflows"] == c0["overflows"] and c1["queries"] - c0["queries"] == NQ
        return got, (c1["candidates"] - c0["candidates"]) / NQ, cl.get_stat("cl_row_classes")

    try:
        got32, n32, cls32 = per_query(32)
        got16, n16, cls16 = per_query(16)
    finally:
        cl.set_option("cl_classes", 0)
    print("candidates per query: 32 classes %.1f, 16 classes %.1f" % (n32, n16))
    assert (cls32, cls16) == (32, 16)
    ref = ex.search(data[1], 10)
    assert _same(got32, ref) and _same(got16, ref)
    assert n32 < n16
