"""Non-finite scores in the scanning coded kinds -- PQ<M>, SQ8, IVF<n>,PQ<M>, IVF<n>,SQ8, bare and under IDMap -- follow FAISS's heap rule
(csrc/pq_kernels.h "ADMISSION RULE", tests/admission_rule.py): a NaN, and a value not strictly better than +-FLT_MAX, is never a result; its
slot prints (-1, +-FLT_MAX).  Queries holding NaN of both signs, +-inf, 1e30 and 1.5e19 go through the C ABI against the CPU models; labels
must be equal and distances equal as uint32.  The cases and their answers are tests/nonfinite_cases.py; that no case is vacuous is asserted
without a GPU in tests/test_admission_rule_cpu.py.  Parameters are set through the accessors: nothing here trains, except the last test,
which is about training sets that hold a NaN or an inf."""
import numpy as np
import pytest

import nonfinite_cases as nfc
import pq_reference as pqr
import sq_reference as sqr
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
FLT_MAX = np.finfo(np.float32).max
STAT = {"pq": "pq", "sq": "sq", "ivfpq": "ivfpq", "ivfsq": "sq"}
KERNEL = {"pq": "pq_scan_kernel", "sq": "sq8_scan_kernel", "ivfpq": "ivfpq_scan_kernel", "ivfsq": "sq8_scan_kernel"}


def _mf():
    import mi355_faiss as mf

    return mf


def _same(D, I, Dr, Ir, what):
    bad = np.argwhere(I != Ir)
    assert bad.size == 0, f"{what}: labels differ in {len(bad)} slots, first (query, slot) {bad[0].tolist()}: {I[tuple(bad[0])]} for {Ir[tuple(bad[0])]}"
    bad = np.argwhere(D.view(np.uint32) != Dr.view(np.uint32))
    assert bad.size == 0, f"{what}: distances differ in {len(bad)} slots, first (query, slot) {bad[0].tolist()}: {D[tuple(bad[0])]} for {Dr[tuple(bad[0])]}"


def _set_parameters(ix, c):
    if c["ivf"]:
        ix.ivf_set_centroids(c["cent"])
    if c["family"].endswith("pq"):
        ix.pq_set_centroids(c["cb"])
    else:
        ix.sq_set_trained(c["vmin"], c["vdiff"])
    assert ix.is_trained


def _check_batch(ix, c, metric, expected, what, nprobe=0):
    xq = c["xq"]
    for k in nfc.KS:
        D, I = ix.search(xq, k, nprobe=nprobe) if nprobe else ix.search(xq, k)
        Dr, Ir = expected(k)
        _same(D, I, Dr, Ir, f"{what} k={k}")
        assert not np.isnan(D).any()
        assert ((I == -1) == (D == (FLT_MAX if metric == L2 else -FLT_MAX))).all()  # a padded slot prints -1, never a label
        for q in nfc.COPIES:  # hostile neighbours in the interleaved group change nothing
            assert np.array_equal(I[q], I[0]) and np.array_equal(D[q].view(np.uint32), D[0].view(np.uint32)), f"{what} k={k}: q{q} differs from q0"
        assert (I[0] >= 0).all()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("kind", sorted(nfc.KINDS) + list(nfc.IDMAP_KINDS))
def test_non_finite_scores_follow_the_heap_rule(kind, metric):
    mf = _mf()
    base = nfc.base_kind(kind)
    c = nfc.inputs(base)
    ix = mf.index_factory(c["d"], kind, metric)
    _set_parameters(ix, c)
    assert ix.get_stat(STAT[c["family"]] + "_rows_per_workgroup") == nfc.R
    if kind == base:
        ix.add(c["xb"])
    else:
        ix.add_with_ids(c["xb"], c["ids"])
    assert ix.ntotal == c["xb"].shape[0]
    _check_batch(ix, c, metric, lambda k: nfc.expected(kind, metric, k), f"{kind} metric={metric}", nprobe=2 if c["ivf"] else 0)
    assert ix.last_kernel_info()["name"] == KERNEL[c["family"]]
    if metric == IP:  # the +inf rows are admitted and come first; the -inf and NaN rows never
        D, I = ix.search(c["xq"], 10, nprobe=2) if c["ivf"] else ix.search(c["xq"], 10)
        n_inf = len(c["planted"])
        assert (D[nfc.Q_INF_POS, :n_inf] == np.inf).all() and (I[nfc.Q_INF_POS, n_inf:] == -1).all()
        assert (D[nfc.Q_INF_NEG] == np.inf).all()
        if not c["ivf"]:
            want = np.asarray(c["planted"])
            assert I[nfc.Q_INF_POS, :n_inf].tolist() == (want if kind == base else c["ids"][want]).tolist()
    for q in (nfc.Q_NAN_POS, nfc.Q_NAN_NEG):
        D, I = ix.search(c["xq"][q : q + 1], 10, nprobe=2) if c["ivf"] else ix.search(c["xq"][q : q + 1], 10)  # (alone: a batch of one)
        assert (I == -1).all() and (D == (FLT_MAX if metric == L2 else -FLT_MAX)).all()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("kind", sorted(nfc.N_OVERFLOW))
def test_non_finite_scores_when_buckets_overflow_and_ranges_are_rescanned(kind, metric, tmp_path):
    """the hostile batch on rows arranged best-last for the controls (codes written through an index file): the same rule, and the statistic
    shows a repeated scan"""
    mf = _mf()
    c = nfc.overflow_inputs(kind, metric)
    path = str(tmp_path / "best_last.index")
    if c["family"] == "pq":
        pqr.write_pq(path, c["d"], metric, c["cb"], c["codes"])
    else:
        sqr.write_sq(path, c["d"], metric, c["vmin"], c["vdiff"], c["codes"])
    ix = mf.read_index(path)
    assert ix.ntotal == c["n"] and ix.is_trained and ix.metric_type == metric
    stat = STAT[c["family"]]
    for k in nfc.KS:
        D, I = ix.search(c["xq"], k)
        _same(D, I, *nfc.overflow_expected(kind, metric, k), f"{kind} best-last metric={metric} k={k}")
        assert ix.get_stat(stat + "_scan_rescans") >= 1
        assert ix.get_stat(stat + "_scan_launches") > ix.get_stat(stat + "_scan_rescans")
        assert ((I == -1) == (D == (FLT_MAX if metric == L2 else -FLT_MAX))).all()
        for q in nfc.COPIES:
            assert np.array_equal(I[q], I[0]) and np.array_equal(D[q].view(np.uint32), D[0].view(np.uint32))
        assert I[0, 0] >= c["n"] - 2 * nfc.R  # the controls' best rows are late ones


@pytest.mark.parametrize("desc,d", [("PQ4", 8), ("IVF4,PQ2", 8), ("IVF4,SQ8", 8)])
def test_a_training_set_with_a_nan_or_an_inf_is_refused(desc, d):
    mf = _mf()
    rng = np.random.default_rng(d + len(desc))
    x = rng.standard_normal((2000, d)).astype(np.float32)
    for bad in (np.nan, np.inf):
        ix = mf.index_factory(d, desc, L2)
        xb = x.copy()
        xb[1234, 0] = bad
        with pytest.raises(mf.FaissException, match="input contains NaN's or Inf's"):
            ix.train(xb)
        assert not ix.is_trained and ix.ntotal == 0
        with pytest.raises(mf.FaissException, match="is_trained"):
            ix.add(x[:10])
    ix = mf.index_factory(d, desc, L2)
    ix.train(x)  # the same rows without the bad value train
    assert ix.is_trained
