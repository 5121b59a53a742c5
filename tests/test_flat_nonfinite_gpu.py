"""Non-finite scores in the Flat-backed kinds -- Flat, IVF<n>,Flat, bare and under IDMap, search and range_search -- against the CPU oracle's
literal heap: rows AND queries holding NaN of both signs, +-inf, 1e30, 1.5e19 and 1e-20-scaled values.  Labels must be equal and distances
equal as uint32; an empty slot prints (-1, +-FLT_MAX), never a label and never a NaN.  The cases and the oracle's answers are
tests/flat_nonfinite_cases.py; that no case is vacuous is asserted without a GPU in tests/test_flat_nonfinite_cases_cpu.py.  Every case
names the kernel that must have served it."""
import functools

import numpy as np
import pytest

import flat_nonfinite_cases as fc
import range_reference as rr
from flat_nonfinite_cases import IP, L2
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FLT_MAX = fc.FLT_MAX
PAIR_SCAN = "flat_pair_scan (ivf_scan_kernel)"
DESCS = ("Flat", "IDMap,Flat")


def _mf():
    import mi355_faiss as mf

    return mf


def _same(D, I, Dr, Ir, what):
    bad = np.argwhere(I != Ir)
    assert bad.size == 0, f"{what}: labels differ in {len(bad)} slots, first (query, slot) {bad[0].tolist()}: {I[tuple(bad[0])]} for {Ir[tuple(bad[0])]}\n got {I[bad[0][0]]}\n ref {Ir[bad[0][0]]}\n got {D[bad[0][0]]}\n ref {Dr[bad[0][0]]}"
    bad = np.argwhere(D.view(np.uint32) != Dr.view(np.uint32))
    assert bad.size == 0, f"{what}: distances differ in {len(bad)} slots, first (query, slot) {bad[0].tolist()}: {D[tuple(bad[0])]} for {Dr[tuple(bad[0])]}"


def _check(D, I, Dr, Ir, metric, what, copies=()):
    _same(D, I, Dr, Ir, what)
    assert not np.isnan(D).any(), what
    assert ((I == -1) == (D == fc.neutral(metric))).all(), what  # an empty slot prints -1, never a label -- nor id_map[-1]
    for q in copies:  # hostile neighbours in the batch change nothing
        assert np.array_equal(I[q], I[0]) and np.array_equal(D[q].view(np.uint32), D[0].view(np.uint32)), f"{what}: q{q} differs from q0"


def _copies(nq):
    return tuple(q for q in fc.COPIES if q < nq)


@functools.lru_cache(maxsize=None)
def _flat_index(desc, case, d, metric):
    c = fc.flat_inputs(case, d)
    ix = _mf().index_factory(d, desc, metric)
    ix.set_option("prefilter", 0)  # the exact kernels are under test: no coarse filter, no shadow store
    ix.set_option("flat_shadow", 0)
    if desc == "Flat":
        ix.add(c["xb"])
    else:
        ix.add_with_ids(c["xb"], c["ids"])
    assert ix.ntotal == fc.N
    return ix


def _flat_search(desc, case, d, metric, nq, k, sel=None, staged=0):
    ix = _flat_index(desc, case, d, metric)
    xq = fc.flat_inputs(case, d)["xq"][:nq]
    ix.set_option("force_staged", staged)
    try:
        D, I = ix.search(xq, k, sel=sel)
    finally:
        ix.set_option("force_staged", 0)
    info = ix.last_kernel_info()
    Dr, Ir = fc.expected(case, metric, k, nq, d, idmap=desc != "Flat", sel=sel)
    _check(D, I, Dr, Ir, metric, f"{desc} {case} d={d} metric={metric} nq={nq} k={k} sel={sel is not None} [{info['name']}]", _copies(nq))
    return info, D, I


flat_cases = pytest.mark.parametrize("desc,case,d,metric", [(desc, case, d, metric) for desc in DESCS for case in fc.CASES for d in fc.DIMS for metric in (L2, IP)])


@flat_cases
def test_flat_fused_kernel(desc, case, d, metric):
    """24 queries (the BLAS branch) at k = 1, 10 and 100 -- 100 is the reservoir rule, and under inner product the query with -inf in H is tied
    at +inf across the split boundary: resolve_ip_ties and the reservoir replay -- and 12 queries under inner product"""
    for k in (1, 10, 100):
        info, D, I = _flat_search(desc, case, d, metric, fc.NQ, k)
        assert info["name"] == "flat_mfma_kernel", info
        assert info["nsplit"] >= 2 and fc.BOUNDARY % fc.split_rows(fc.N, d, info["nsplit"]) == 0, info  # hostile rows on both sides of a split
        if metric == IP:
            assert (D[fc.Q_INF_NEG] == np.inf).all()
            n_adm = len(fc.flat_inputs(case, d)["planted"])
            assert (D[fc.Q_INF_POS, : min(k, n_adm)] == np.inf).all() and (I[fc.Q_INF_POS, n_adm:] == -1).all()
        for q in (fc.Q_NAN_POS, fc.Q_NAN_NEG):
            assert (I[q] == -1).all()
    if metric == IP:
        info, _, _ = _flat_search(desc, case, d, metric, 12, fc.K)
        assert info["name"] == "flat_mfma_kernel", info


@flat_cases
def test_flat_direct_kernel_and_pair_scan(desc, case, d, metric):
    info, _, _ = _flat_search(desc, case, d, metric, fc.NQ, 300)  # beyond the fused kernel's 256
    assert info["name"] == "flat_direct_kernel", info
    info, _, _ = _flat_search(desc, case, d, metric, 3, fc.K)  # the streaming kernel of <= 4 queries: one control, two hostile
    assert info["name"] == "flat_direct_kernel", info
    info, _, _ = _flat_search(desc, case, d, metric, 7, fc.K, staged=1)
    assert info["name"] == "flat_direct_kernel", info
    info, _, _ = _flat_search(desc, case, d, metric, 7, fc.K)
    assert info["name"] == PAIR_SCAN, info


@flat_cases
def test_flat_selector_instances(desc, case, d, metric):
    """IDSelectorBatch keeping about 40 % of the rows, some hostile rows among them: L2 takes the per-pair arithmetic, inner product stays on
    the fused kernel"""
    keep = fc.keep_rows(case, d)
    sel = ("batch", keep if desc == "Flat" else fc.flat_inputs(case, d)["ids"][keep])
    for nq in (fc.NQ, 7):
        info, D, I = _flat_search(desc, case, d, metric, nq, fc.K, sel=sel)
        assert np.isin(I[I >= 0], sel[1]).all()
        if metric == L2 or nq == 7:
            assert info["name"] == PAIR_SCAN, info
        else:
            assert info["name"] == "flat_mfma_kernel", info


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("case", fc.CASES)
def test_flat_two_calls_equal_one(case, metric):
    """the batch twice in one call against two calls over the same index: the scratch buffers of a batch that left slots empty are reused"""
    d = 20
    ix = _flat_index("IDMap,Flat", case, d, metric)
    xq = fc.flat_inputs(case, d)["xq"]
    Dr, Ir = fc.expected(case, metric, fc.K, fc.NQ, d, idmap=True)
    D2, I2 = ix.search(np.concatenate([xq, xq]), fc.K)
    assert ix.last_kernel_info()["name"] == "flat_mfma_kernel"
    Da, Ia = ix.search(xq, fc.K)
    Db, Ib = ix.search(xq[::-1].copy(), fc.K)  # (the hostile queries now sit in other places of the buffers)
    _check(Da, Ia, Dr, Ir, metric, "first call")
    _check(Db[::-1], Ib[::-1], Dr, Ir, metric, "second call")
    _check(D2, I2, np.concatenate([Dr, Dr]), np.concatenate([Ir, Ir]), metric, "one call")


# ---------------------------------------------------------------------------------------------------------------------------- IVF2,Flat
def _ivf_index(metric, d, idmap):
    c = fc.ivf_inputs(metric, d)
    g = _mf().index_factory(d, ("IDMap," if idmap else "") + "IVF2,Flat", metric)
    g.ivf_set_centroids(c["cent"])
    if idmap:
        g.add_with_ids(c["xb"], c["ids"])
    else:
        g.add(c["xb"])
    assert g.ntotal == fc.N_IVF  # (the NaN rows count, though no list holds them)
    return g


IVF_MODES = {  # options on top of ivf_collect = 0 -> the kernel's reported name
    "scan": (dict(ivf_mfma=0), "ivf_scan_kernel"),
    "items": (dict(ivf_mfma=0, ivf_fast_scan=0), "ivf_list_scan (flat_direct_kernel items)"),
    "select": (dict(ivf_mfma=0, ivf_select=1), "ivf_select (all distances + segmented sort)"),
    "mfma": (dict(), "ivf_mfma_scan"),  # inner product at d = 128 only: its default without the filter
}


@pytest.mark.parametrize("idmap", [False, True])
@pytest.mark.parametrize("d", fc.IVF_DIMS)
@pytest.mark.parametrize("metric", [L2, IP])
def test_ivf_exact_kernels(metric, d, idmap):
    """NaN, +inf and -inf scores INSIDE the list scans (under L2 the +inf of (2.8e19)^2 against rows whose list has a finite coarse value),
    queries with no probe at all and with one probe and one -1"""
    g = _ivf_index(metric, d, idmap)
    xq = fc.ivf_inputs(metric, d)["xq"]
    g.set_option("ivf_collect", 0)
    for mode, (options, name) in IVF_MODES.items():
        if mode == "mfma" and (metric != IP or d != 128):  # (a shape of test_ivf_inner_product_scans_on_the_mfma_kernel_bit_exact)
            continue
        for key, v in options.items():
            g.set_option(key, v)
        for nprobe in (1, 2):
            for k in (1, fc.K):
                D, I = g.search(xq, k, nprobe=nprobe)
                got = g.last_kernel_info()["name"]
                assert got.startswith(name), (mode, got)
                Dr, Ir = fc.ivf_expected(metric, d, k, nprobe, idmap)
                _check(D, I, Dr, Ir, metric, f"IVF2,Flat idmap={idmap} d={d} metric={metric} {mode} nprobe={nprobe} k={k}", fc.COPIES)
                for q in (fc.Q_NAN_POS, fc.Q_NAN_NEG, fc.Q_NO_COARSE):
                    assert (I[q] == -1).all()
        for key in options:
            g.set_option(key, {"ivf_mfma": -1, "ivf_fast_scan": 1, "ivf_select": 0}[key])


def _filter_search(metric, nlist, n, m, k, nprobe, cl_big=None):
    c = fc.filter_inputs(metric, nlist, n, m)
    g = _mf().index_factory(fc.FILTER_D, f"IVF{nlist},Flat", metric)
    g.ivf_set_centroids(c["cent"])
    g.add(c["xb"])
    assert g.ntotal == n
    if cl_big is not None:
        g.set_option("ivf_cl_big", cl_big)
    D, I = g.search(c["xq"], k, nprobe=nprobe)
    assert g.last_kernel_info()["name"] == "ivf_bf16_collect_kernel", g.last_kernel_info()
    Dr, Ir = c["oracle"].search(c["xq"], k, nprobe=nprobe)
    _check(D, I, Dr, Ir, metric, f"IVF{nlist},Flat on the coarse filter metric={metric} m={m} k={k} ivf_cl_big={cl_big}")
    assert not np.isin(I[: fc.FILTER_HOSTILE], np.arange(m)).any()  # a row that scores NaN is never a result
    if m:  # the queries that probe the list with the inf rows have no finite bound: the exact paths answered them, the filter the others
        assert fc.FILTER_HOSTILE <= g.prefilter_stats()["fallback_queries"] < fc.FILTER_NQ
    assert (I[fc.FILTER_Q_NAN] == -1).all()


@pytest.mark.parametrize("metric,m", [(L2, 0), (IP, 0), (IP, 1), (IP, 9)])
def test_ivf_coarse_filter_small_lists(metric, m):
    _filter_search(metric, 16, 20000, m, 10, 4)


@pytest.mark.parametrize("cl_big", [1, 2])
@pytest.mark.parametrize("metric,m", [(L2, 0), (IP, 1), (IP, 32), (IP, 33)])
def test_ivf_coarse_filter_big_lists_with_nan_rows_in_the_bound_sample(metric, m, cl_big):
    """k = 33: the frozen bound B comes from the first 256 rows of the nearest lists (ivf_big_bound_direct_kernel, ivf_cl_big = 1) or from all of
    them (2).  m rows with +inf in H are the first arrivals of the list the hostile queries probe first and score 0 * inf = NaN against them.
    Keyed by its sign a NaN would be the BEST of the sample: with m = k - 1 the bound would be the best real sampled value and cut about 30 of
    the 33 results (tests/test_flat_nonfinite_cases_cpu.py prints the count on the oracle).  The kernel now tests the value -- but no input
    can show the difference in a result: the list with the inf rows has no finite largest norm, so every query that probes it has no
    finite error bound, never uses B and is answered by the exact paths (rerun_unproven) while the filter serves the rest of the batch.
    Before that re-run existed one such query sent the whole batch to the older kernels and this case failed on the kernel's name alone.
    The sign of the device's NaN for 0 * inf has therefore not been observed: no output may hold a NaN and none depends on its sign."""
    _filter_search(metric, 32, 40000, m, 33, 8, cl_big)


# ------------------------------------------------------------------------------------------------------------------------- range_search
def _radii(metric, dis):
    finite = dis[np.isfinite(dis)]
    return (np.inf if metric == L2 else -np.inf, np.float32(np.quantile(finite, 0.02 if metric == L2 else 0.98)), fc.neutral(metric))


@pytest.mark.parametrize("desc,case,d,metric", [(desc, case, d, metric) for desc in DESCS[:1] for case in fc.CASES for d in fc.DIMS for metric in (L2, IP)])
def test_flat_range_search(desc, case, d, metric):
    """a NaN distance is never a hit; under inner product with radius -inf a +inf distance is one and a -inf is not; under L2 with radius
    +inf a +inf distance is not (both compares are strict)"""
    ix = _flat_index(desc, case, d, metric)
    ix.set_option("range_mfma", 1)
    c = fc.flat_inputs(case, d)
    for nq, branch in ((fc.NQ, "blas"), (7, "pair")):
        dis = fc.flat_scores(case, d, metric, branch)[:nq]
        for radius in _radii(metric, dis):
            got = ix.range_search(c["xq"][:nq], radius)
            name = ix.last_kernel_info()["name"]
            assert name == ("range_mfma_kernel" if nq >= 20 and d <= 128 else "range_pair_kernel"), name
            want = rr.select(metric, dis, radius)
            assert rr.same(got, want), f"{case} d={d} metric={metric} nq={nq} radius={radius!r}: {got[0][:12]} for {want[0][:12]}"
            assert not np.isnan(got[1]).any()
            assert not (got[1] == (np.inf if metric == L2 else -np.inf)).any()
        assert want[0][-1] > 0  # (the last radius, +-FLT_MAX, admits every finite distance)


@pytest.mark.parametrize("d", fc.IVF_DIMS)
@pytest.mark.parametrize("metric", [L2, IP])
def test_ivf_range_search(metric, d):
    g = _ivf_index(metric, d, False)
    c = fc.ivf_inputs(metric, d)
    with np.errstate(all="ignore"):
        dis = orc.pair_chains(metric, c["xb"], c["xq"])
    for nprobe in (1, 2):
        for radius in _radii(metric, dis):
            got = g.range_search(c["xq"], radius, nprobe=nprobe)
            assert g.last_kernel_info()["name"] == "range_pair_kernel"
            want = fc.ivf_range(metric, d, radius, nprobe)
            assert rr.same(got, want), f"IVF2,Flat d={d} metric={metric} nprobe={nprobe} radius={radius!r}: {got[0][:12]} for {want[0][:12]}"
            assert not np.isnan(got[1]).any()
        assert want[0][-1] > 0
