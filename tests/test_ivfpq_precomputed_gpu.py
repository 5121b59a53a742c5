"""IVF<n>,PQ<M> with the option ivfpq_precomputed_table (include/mi355_faiss.h "precomputed tables"): tables joined from a per-query and a
per-list part instead of built per (query, list) pair.  Inner product: the same chains, so the same bits as the option off on any data.
L2: the same bits wherever every intermediate is exact (small integers), a derived rounding bound against float64 elsewhere."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2, IP = 1, 0
KEY = "ivfpq_precomputed_table"
SHAPES = [(8, 4), (24, 8), (64, 16), (96, 48), (130, 65)]  # every table layout (float4, float2, scalar); dsub 3 is odd
NLIST, NB, NQ, K = 5, 3000, 37, 10  # 37 queries: pair groups of fewer than, exactly and more than Q pairs


def _mf():
    import mi355_faiss as mf

    return mf


@functools.lru_cache(maxsize=None)
def _data(d, M, lattice, nlist=NLIST, nb=NB):
    rng = np.random.default_rng(1000 * d + 2 * M + lattice)
    if lattice:
        draw = lambda *s: rng.integers(-3, 4, size=s).astype(np.float32)
        cent, cb, xb, xq = draw(nlist, d), draw(M, 256, d // M), draw(nb, d), draw(NQ, d)
    else:
        draw = lambda *s: rng.standard_normal(s).astype(np.float32)
        cent, cb = draw(nlist, d), 0.3 * draw(M, 256, d // M)
        xb, xq = cent[rng.integers(0, nlist, nb)] + 0.3 * draw(nb, d), draw(NQ, d)
    for a in (cent, cb, xb, xq):
        a.setflags(write=False)
    return cent, cb, xb, xq


def _build(desc, metric, cent, cb, xb, ids=None):
    ix = _mf().index_factory(cent.shape[1], desc, metric)
    ix.ivf_set_centroids(cent)
    ix.pq_set_centroids(cb)
    ix.add(xb) if ids is None else ix.add_with_ids(xb, ids)
    return ix


@functools.lru_cache(maxsize=None)
def _index(d, M, metric, lattice):
    cent, cb, xb, _ = _data(d, M, lattice)
    return _build(f"IVF{NLIST},PQ{M}", metric, cent, cb, xb)


def _on_off(ix, xq, nprobe, **kw):
    ix.set_option(KEY, 0)
    off = ix.search(xq, K, nprobe=nprobe, **kw)
    ix.set_option(KEY, 1)
    on = ix.search(xq, K, nprobe=nprobe, **kw)
    assert ix.get_stat("ivfpq_query_table_launches") >= 1
    return on, off


def _same(a, b, what):
    assert np.array_equal(a[1], b[1]), f"{what}: labels differ in {(a[1] != b[1]).sum()} slots"
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{what}: distances differ in {(a[0] != b[0]).sum()} slots"


@pytest.mark.parametrize("nprobe", [1, 3, NLIST])
@pytest.mark.parametrize("d,M", SHAPES)
@pytest.mark.parametrize("metric,lattice", [(IP, False), (L2, True)])
def test_option_on_gives_the_bits_of_option_off(metric, lattice, d, M, nprobe):
    on, off = _on_off(_index(d, M, metric, lattice), _data(d, M, lattice)[3], nprobe)
    _same(on, off, "option on against off")


@pytest.mark.parametrize("metric,lattice", [(IP, False), (L2, True)])
def test_one_list_across_two_segment_boundaries(metric, lattice):
    cent, cb, xb, xq = _data(8, 4, lattice, nlist=1, nb=2 * 8192 + 5)
    on, off = _on_off(_build("IVF1,PQ4", metric, cent, cb, xb), xq, 1)
    _same(on, off, "2 * 8192 + 5 rows in one list")


@pytest.mark.parametrize("nprobe", [1, 3, NLIST])
@pytest.mark.parametrize("d,M", SHAPES)
def test_l2_on_random_data_is_within_the_rounding_bound_of_float64(d, M, nprobe):
    """Reference: every stored code decoded (list codes + codebooks + centroid), |x - c - p^|^2 in float64.  The device computes
    b + sum_m fmaf(-2, S, fmaf(2, <c_m, p>, <p, p>)), b = <v, v>, v = x - c: in exact arithmetic the same number.  First-order bound,
    u = 2^-24: a chain of n fmas over a, b errs by at most n u |a| |b| (Cauchy-Schwarz on sum |a_k b_k|), so <p, p>, <c_m, p> and
    <x_m, p> err by dsub u times |p|^2, |c_m||p|, |x_m||p|; the two joining fmas add 2 u of their results, the M + 1 additions of the
    sum M + 1 u of their partial sums, the subtraction in v another 2 u |v_m|^2; every partial result is bounded by the sum of the term
    magnitudes A = sum_m (|v_m|^2 + |p|^2 + 2 |c_m||p| + 2 |x_m||p|).  That gives (dsub + M + 4) u A, the bound the option's issue
    states; b's chain is charged dsub + M + 4 roundings per term like the others.  Labels are compared where the reference's neighbouring
    distances are more than twice the bound apart, which must be at least 90 % of the slots."""
    cent, cb, xb, xq = _data(d, M, False)
    ix = _index(d, M, L2, False)
    ix.set_option(KEY, 1)
    D, I = ix.search(xq, K, nprobe=nprobe)
    dsub, gamma = d // M, (d // M + M + 4) * 2.0**-24
    c64, q64 = cent.astype(np.float64), xq.astype(np.float64)
    probes = np.argsort(((q64[:, None, :] - c64[None]) ** 2).sum(-1), axis=1, kind="stable")[:, :nprobe]
    lists = [ix.ivfpq_list(l) for l in range(NLIST)]
    sub = lambda a: a.reshape(*a.shape[:-1], M, dsub)
    compared = worst = 0.0
    for q in range(NQ):
        ids, dist, bound = [], [], []
        for l in probes[q]:
            p = cb.astype(np.float64)[np.arange(M), lists[l][1]]  # [n, M, dsub]
            pn = np.sqrt((p**2).sum(-1))
            v, cn, xn = sub(q64[q] - c64[l]), np.sqrt((sub(c64[l]) ** 2).sum(-1)), np.sqrt((sub(q64[q]) ** 2).sum(-1))
            ids.append(lists[l][0])
            dist.append(((v - p) ** 2).sum((-1, -2)))
            bound.append(gamma * ((v**2).sum(-1) + pn**2 + 2 * cn * pn + 2 * xn * pn).sum(-1))
        ids, dist, bound = map(np.concatenate, (ids, dist, bound))
        order = np.argsort(dist, kind="stable")[: K + 1]
        assert np.isin(I[q], ids).all(), f"query {q}: a label outside the probed lists"
        by_id = np.argsort(ids)
        at = by_id[np.searchsorted(ids[by_id], I[q])]  # where the reference holds the rows the device returned
        err = np.abs(D[q] - dist[at]) / bound[at]
        worst = max(worst, err.max())
        assert err.max() <= 1.0, f"query {q}: distance off by {err.max():.3f} of the bound"
        gap = np.diff(dist[order]) > 2 * np.maximum(bound[order[:-1]], bound[order[1:]])
        clear = np.concatenate(([True], gap[:-1])) & gap  # slot i against slots i - 1 and i + 1 of the reference's order
        assert np.array_equal(I[q][clear], ids[order[:K]][clear]), f"query {q}: labels differ where the reference is decided"
        compared += clear.sum()
    print(f"d={d} M={M} nprobe={nprobe}: worst error {worst:.4f} of the bound, {compared / (NQ * K):.3f} of the slots compared")
    assert compared >= 0.9 * NQ * K


@pytest.mark.parametrize("metric", [L2, IP])
def test_tables_follow_the_centroids_and_the_option_reaches_wrapped_indexes(metric):
    d, M = 24, 8
    cent, cb, xb, xq = _data(d, M, True)
    cent2 = np.ascontiguousarray(cent[::-1] + 1.0)
    ids = np.arange(NB, dtype=np.int64) * 3 + 7
    ix = _build(f"IDMap,IVF{NLIST},PQ{M}", metric, cent, cb, xb, ids)
    assert ix.get_stat("ivfpq_precomputed_bytes") == 0
    ix.set_option(KEY, 1)  # (through IDMap)
    assert ix.get_stat("ivfpq_precomputed_bytes") == 0  # built by the first search that needs it
    ix.search(xq, K, nprobe=3)
    assert ix.get_stat("ivfpq_query_table_launches") >= 1
    assert ix.get_stat("ivfpq_precomputed_bytes") == (NLIST * M * 1024 if metric == L2 else 0)
    assert ix.remove_ids(("batch", ids)) == NB and ix.ntotal == 0
    ix.ivf_set_centroids(cent2)  # the per-list table is stale now
    ix.add_with_ids(xb, ids)
    fresh = _build(f"IDMap,IVF{NLIST},PQ{M}", metric, cent2, cb, xb, ids)
    sel = ("batch", ids[::2])
    _same(ix.search(xq, K, nprobe=3), fresh.search(xq, K, nprobe=3), "after new centroids against a fresh index, option off")
    _same(ix.search(xq, K, nprobe=3, sel=sel), fresh.search(xq, K, nprobe=3, sel=sel), "the same under a batch selector")
    ix.set_option(KEY, 0)
    assert ix.get_stat("ivfpq_precomputed_bytes") == 0
    _same(ix.search(xq, K, nprobe=3), fresh.search(xq, K, nprobe=3), "option off again")


@pytest.mark.parametrize("desc,value,text", [("IVF5,PQ4", 2, "ivfpq_precomputed_table = 2"), ("IVF5,PQ4", -1, "= -1"), ("Flat", 1, "unknown option")])
def test_refusals(desc, value, text):
    mf = _mf()
    with pytest.raises(mf.FaissException, match=text):
        mf.index_factory(8, desc, L2).set_option(KEY, value)
