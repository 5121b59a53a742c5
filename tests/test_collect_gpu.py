"""bf16 coarse filter + exact f32 re-scoring (csrc/flat_collect.hip, option prefilter = 2) behind IndexFlat::search
(src/faiss_extension.cpp:631): ONE bf16 product per element pair selects candidates by a proven bound; the answers must
be those of the exact f32 kernel and of the oracle's BLAS branch BIT FOR BIT -- labels and distances -- on friendly data,
on duplicate-heavy data (every tied row is a candidate: no fall back needed), on non-finite input (those queries are
re-run on the exact kernel), for both metrics, with inner-product boundary ties, through IDMap."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
KERNEL = "flat_bf16_collect_kernel"


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss

    return mi355_faiss


def _pair(mf, d, metric, xb, desc="Flat", ids=None):
    cl, ex = mf.index_factory(d, desc, metric), mf.index_factory(d, desc, metric)
    cl.set_option("prefilter", 2)
    ex.set_option("prefilter", 0)
    for ix in (cl, ex):
        for i0 in range(0, len(xb), 1 << 16):
            if ids is None:
                ix.add(xb[i0 : i0 + (1 << 16)])
            else:
                ix.add_with_ids(xb[i0 : i0 + (1 << 16)], ids[i0 : i0 + (1 << 16)])
    return cl, ex


def _check(cl, ex, xq, k, metric, xb=None, oracle_rows=0, overflow=False):
    D1, I1 = cl.search(xq, k)
    # (a batch whose candidate stream overflows is handed to the bf16x3 path)
    assert cl.last_kernel_info()["name"] in (("flat_bf16x3_kernel", KERNEL) if overflow else (KERNEL,))
    D0, I0 = ex.search(xq, k)
    # (FAISS's per-pair branch -- L2 with fewer than 20 queries -- has its own exact kernel)
    assert ex.last_kernel_info()["name"] == "flat_mfma_kernel" or (len(xq) < 20 and metric == L2)
    assert np.array_equal(I1, I0), "labels differ from the exact f32 kernel"
    assert np.array_equal(D1.view(np.uint32), D0.view(np.uint32)), "distances differ from the exact f32 kernel"
    if oracle_rows:
        # (the whole batch decides FAISS's branch: BLAS from 20 queries on, per pair below)
        Do, Io = orc.flat_search(metric, xb, xq[:oracle_rows], k, force_path=orc.PATH_BLAS if len(xq) >= 20 else orc.PATH_PAIR)
        assert np.array_equal(I1[:oracle_rows], Io) and np.array_equal(D1[:oracle_rows].view(np.uint32), Do.view(np.uint32))
    return D1, I1


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,nb,nq,k", [(128, 200_000, 700, 10), (100, 99_991, 257, 1), (128, 70_000, 1100, 15), (65, 50_000, 64, 10),
                                       (128, 33_000, 20, 4),
                                       # 16 < d <= 64: the same 128-dim bf16 store, zero-padded; f32 rows of pitch 64 / 32
                                       (64, 120_000, 600, 10), (48, 80_000, 300, 7), (32, 150_000, 520, 10), (20, 60_000, 90, 3),
                                       (64, 70_000, 16, 5), (33, 66_000, 300, 20)])
def test_collect_equals_exact_kernel_and_oracle(mf, metric, d, nb, nq, k):
    rs = np.random.RandomState(d + nb)
    xb = rs.rand(nb, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xq = rs.rand(nq, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    cl, ex = _pair(mf, d, metric, xb)
    _check(cl, ex, xq, k, metric, xb, oracle_rows=64)
    st = cl.collect_stats()
    assert st["queries"] == nq and st["overflows"] == 0 and st["candidates"] >= nq * min(k, nb), st
    assert cl.prefilter_stats()["fallback_queries"] == 0


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,nb,nq,k", [(128, 150_000, 600, 20), (128, 80_000, 300, 31), (96, 60_000, 150, 17), (128, 40_000, 40, 24)])
def test_k_up_to_32_takes_the_coarse_filter_with_32_row_classes(mf, metric, d, nb, nq, k):
    """16 < k <= 32 at d <= 128: 32 class slots per query (row & 31), the bound is the k-th best of them; same kernel, same
    re-scoring, same answers as the exact f32 kernel and the oracle.  (Inner product searches k + 1 for the tie detection:
    k <= 31.)  Small batches take the workgroup kernel here (the one-wavefront-per-segment kernel keeps 16 classes)."""
    rs = np.random.RandomState(k * 1000 + d)
    xb = rs.rand(nb, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xq = rs.rand(nq, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xb[::53] = xb[11]  # duplicates: ties inside the result lists
    cl, ex = _pair(mf, d, metric, xb)
    _check(cl, ex, xq, k, metric, xb, oracle_rows=48)
    st = cl.collect_stats()
    assert st["queries"] == nq and st["overflows"] == 0, st
    cl.set_option("cl_k32", 0)  # the round-2 route for these k: bf16x3 prefilter / exact kernel
    D2, I2 = cl.search(xq, k)
    assert cl.last_kernel_info()["name"] != KERNEL
    D1, I1 = ex.search(xq, k)
    assert np.array_equal(I2, I1) and np.array_equal(D2.view(np.uint32), D1.view(np.uint32))


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,nb,nq,k", [(128, 150_000, 600, 64), (128, 90_000, 300, 100), (96, 70_000, 150, 33), (128, 50_000, 40, 127),
                                       (64, 120_000, 200, 128)])
def test_k_up_to_128_takes_the_coarse_filter_with_four_subsets_of_32_classes(mf, metric, d, nb, nq, k):
    """32 < k <= 128 at d <= 128 (round 4; VERDICT r3 missing #6: these k fell to the bf16x3 prefilter up to 40 and to the f32
    kernel beyond, 5-12x slower): 128 class slots per query (row & 127) in four subsets of 32; the bound is the WORST of the
    subsets' ceil(k / 4)-th best class values -- at least k distinct rows are that good.  Same scan kernel, same re-scoring, same
    answers as the exact f32 kernel and the oracle (whose k >= 100 results come out of FAISS's reservoir; inner product searches
    k + 1 for the tie detection, so k = 128 stays on the exact kernels there)."""
    rs = np.random.RandomState(k * 1000 + d)
    xb = rs.rand(nb, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xq = rs.rand(nq, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xb[::53] = xb[11]  # duplicates: ties inside the result lists
    cl, ex = _pair(mf, d, metric, xb)
    if metric == IP and k + 1 > 128:
        # (round 6: k + 1 = 129 entries are a "big list" -- served by the filter's range bounds on stores of >= 65 536 rows)
        D, I = cl.search(xq, k)
        assert (cl.last_kernel_info()["name"] == KERNEL) == (nb >= 65536 and nb >= 64 * k)
        De, Ie = ex.search(xq, k)
        assert np.array_equal(I, Ie) and np.array_equal(D.view(np.uint32), De.view(np.uint32))
        return
    _check(cl, ex, xq, k, metric, xb, oracle_rows=48)
    st = cl.collect_stats()
    assert st["queries"] == nq and st["overflows"] == 0, st


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,nb,nq,k", [(128, 300_000, 300, 129), (128, 300_000, 200, 200), (96, 280_000, 64, 500), (128, 300_000, 1100, 1000),
                                       (64, 530_000, 40, 2048), (128, 300_000, 12, 300), (128, 270_000, 256, 128),
                                       # small stores (>= 64 rows per entry asked for) and lists beyond 2048 (up to what the exact kernels could serve as a fall-back)
                                       (128, 70_000, 100, 1000), (64, 300_000, 24, 3000)])
def test_lists_beyond_128_entries_stay_on_the_coarse_filter(mf, metric, d, nb, nq, k):
    """round 6 (VERDICT r5 missing #3; the reference's post-filter use asks for k in the hundreds and thousands, README.md:222-271,
    go/main_test.go:26-32): k > 128 at d <= 128 -- bounds from ceil(k / 64) row ranges' class slots (pass A over a quarter of the rows),
    the scan against those bounds frozen, exact re-scoring, one segmented sort per batch.  Same answers as the exact kernels and the
    oracle (FAISS's reservoir from k = 100 on; inner product searches k + 1 entries: k = 128 is a big list there)."""
    rs = np.random.RandomState(k * 1000 + d)
    xb = rs.rand(nb, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xq = rs.rand(nq, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xb[::53] = xb[11]  # duplicates: ties inside the result lists
    cl, ex = _pair(mf, d, metric, xb)
    D1, I1 = cl.search(xq, k)
    assert cl.last_kernel_info()["name"] == KERNEL, cl.last_kernel_info()
    D0, I0 = ex.search(xq, k)
    assert ex.last_kernel_info()["name"] != KERNEL
    assert np.array_equal(I1, I0), "labels differ from the exact kernels"
    assert np.array_equal(D1.view(np.uint32), D0.view(np.uint32)), "distances differ from the exact kernels"
    no = min(nq, 6)
    Do, Io = orc.flat_search(metric, xb, xq[:no], k, force_path=orc.PATH_BLAS if nq >= 20 else orc.PATH_PAIR)
    assert np.array_equal(I1[:no], Io) and np.array_equal(D1[:no].view(np.uint32), Do.view(np.uint32))
    st = cl.collect_stats()
    assert st["queries"] == nq and st["candidates"] >= nq * k and st["candidates"] < nq * nb * 0.5, st
    cl.set_option("cl_bigk", 0)  # (the switch: the exact kernels as before)
    D2, I2 = cl.search(xq[:32], k)
    assert (cl.last_kernel_info()["name"] != KERNEL) == (k > 128 or metric == IP)
    assert np.array_equal(I2, I0[:32]) or nq < 20  # (a batch of < 20 takes FAISS's per-pair branch: other last bits)


def test_big_list_with_selector_and_idmap(mf):
    rs = np.random.RandomState(79)
    d, nb, k = 128, 280_000, 400
    xb = rs.randint(-2, 3, size=(nb, d)).astype(np.float32)  # integer rows: exact ties everywhere, also at the k-th value
    xq = rs.randint(-2, 3, size=(48, d)).astype(np.float32)
    ids = (rs.permutation(3 * nb)[:nb] + 3).astype(np.int64)
    keep = ids[rs.rand(nb) < 0.5]
    for metric in (L2, IP):
        g, o = mf.index_factory(d, "IDMap,Flat", metric), orc.Index(d, "IDMap,Flat", metric)
        g.set_option("prefilter", 2)
        for a in (g, o):
            a.add_with_ids(xb, ids)
        for sel in (None, ("batch", keep)):
            D, I = g.search(xq, k, sel=sel)
            Do, Io = o.search(xq[:4], k, sel=sel)
            assert np.array_equal(D[:4].view(np.uint32), Do.view(np.uint32)), (metric, sel and sel[0], g.last_kernel_info())
            assert np.array_equal(I[:4], Io), (metric, sel and sel[0])


@pytest.mark.parametrize("metric", [L2, IP])
def test_k_100_with_selector_and_idmap_on_the_coarse_filter(mf, metric):
    rs = np.random.RandomState(77)
    d, nb, k = 128, 70_000, 100
    xb = rs.randint(-2, 3, size=(nb, d)).astype(np.float32)  # integer rows: exact ties everywhere, also at the k-th value
    xq = rs.randint(-2, 3, size=(120, d)).astype(np.float32)
    ids = (rs.permutation(3 * nb)[:nb] + 3).astype(np.int64)
    g, o = mf.index_factory(d, "IDMap,Flat", metric), orc.Index(d, "IDMap,Flat", metric)
    g.set_option("prefilter", 2)
    for a in (g, o):
        a.add_with_ids(xb, ids)
    keep = ids[rs.rand(nb) < 0.5]
    for sel in (None, ("batch", keep)):
        D, I = g.search(xq, k, sel=sel)
        assert g.last_kernel_info()["name"] == KERNEL
        Do, Io = o.search(xq, k, sel=sel)
        assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), sel and sel[0]
        assert np.array_equal(I, Io), sel and sel[0]


@pytest.mark.parametrize("metric", [L2, IP])
def test_duplicates_and_ties_need_no_fall_back(mf, metric):
    """40 distinct vectors repeated 100k times: every row tied at the k-th value is a candidate -- 2 500 copies of each of
    the nearest vectors, more than the candidate stream holds: the batch overflows and the bf16x3 path (and behind it the
    exact kernel) serves it.  Mixed data: the tied rows are all candidates and the exact (value, id) order decides."""
    rs = np.random.RandomState(5)
    base = rs.rand(40, 128).astype(np.float32)
    xb = base[rs.randint(0, 40, 100_000)]
    xq = rs.rand(300, 128).astype(np.float32)
    cl, ex = _pair(mf, 128, metric, xb)
    _check(cl, ex, xq, 10, metric, xb, oracle_rows=32, overflow=True)
    xb2 = rs.rand(120_000, 128).astype(np.float32)
    xb2[rs.randint(0, 120_000, 30_000)] = xb2[rs.randint(0, 120_000, 30_000)]
    xq2 = np.concatenate([rs.rand(200, 128).astype(np.float32), xb2[rs.randint(0, 120_000, 200)]])
    cl, ex = _pair(mf, 128, metric, xb2)
    _check(cl, ex, xq2, 10, metric, xb2, oracle_rows=400)


def test_idmap_and_integer_inner_product_ties(mf):
    rs = np.random.RandomState(9)
    xb = rs.randint(-3, 4, size=(80_000, 100)).astype(np.float32)
    xq = rs.randint(-3, 4, size=(256, 100)).astype(np.float32)
    ids = (rs.permutation(400_000)[:80_000] + 11).astype(np.int64)
    cl, ex = _pair(mf, 100, IP, xb, desc="IDMap,Flat", ids=ids)
    D, I = _check(cl, ex, xq, 10, IP)
    o = orc.Index(100, "IDMap,Flat", IP)
    o.add_with_ids(xb, ids)
    Do, Io = o.search(xq, 10)
    assert np.array_equal(I, Io) and np.array_equal(D, Do)


@pytest.mark.parametrize("metric", [L2, IP])
def test_non_finite_and_huge_values(mf, metric):
    rs = np.random.RandomState(2)
    xb = rs.rand(60_000, 128).astype(np.float32)
    xq = rs.rand(128, 128).astype(np.float32)
    xq[3, 1] = np.nan
    xq[4] *= 1e19
    xq[5, 0] = np.inf
    cl, ex = _pair(mf, 128, metric, xb)
    D1, I1 = cl.search(xq, 10)
    assert cl.last_kernel_info()["name"] == KERNEL
    D0, I0 = ex.search(xq, 10)
    assert np.array_equal(I1, I0) and np.array_equal(D1.view(np.uint32), D0.view(np.uint32))
    assert 2 <= cl.prefilter_stats()["fallback_queries"] <= 3  # only the queries without a finite bound are re-run
    with np.errstate(all="ignore"):  # the oracle's literal heap: the hostile queries and the first 16 (the exact kernel alone is no reference)
        Do, Io = orc.flat_search(metric, xb, xq, 10, force_path=orc.PATH_BLAS)
    for q in sorted(set(range(16)) | {3, 4, 5}):
        assert np.array_equal(I1[q], Io[q]) and np.array_equal(D1[q].view(np.uint32), Do[q].view(np.uint32)), q
    assert not np.isnan(D1).any()
    xb[100, 5] = np.nan
    xb[200, 7] = np.inf
    xb[300] *= 1e18
    xb[400] *= 1e-20
    cl, ex = _pair(mf, 128, metric, xb)  # a row norm overflows: no finite bound for anybody, everything is re-run
    D1, I1 = cl.search(xq, 10)
    D0, I0 = ex.search(xq, 10)
    assert np.array_equal(I1, I0) and np.array_equal(D1.view(np.uint32), D0.view(np.uint32))
    with np.errstate(all="ignore"):  # the oracle's literal heap: now with hostile rows too
        Do, Io = orc.flat_search(metric, xb, xq, 10, force_path=orc.PATH_BLAS)
    for q in sorted(set(range(16)) | {3, 4, 5}):
        assert np.array_equal(I1[q], Io[q]) and np.array_equal(D1[q].view(np.uint32), Do[q].view(np.uint32)), q
    assert not np.isnan(D1).any()


def test_large_norm_offset_data(mf):
    """rows far from the origin: the store is centred on the mean row, so the bound scales with the spread of the data and
    not with its offset -- no flood of candidates"""
    rs = np.random.RandomState(12)
    xb = (rs.rand(80_000, 128).astype(np.float32) + 3.0)
    xq = (rs.rand(100, 128).astype(np.float32) + 3.0)
    cl, ex = _pair(mf, 128, L2, xb)
    _check(cl, ex, xq, 10, L2, xb, oracle_rows=32)
    st = cl.collect_stats()
    assert st["overflows"] == 0 and st["candidates"] < 100 * 4096, st
    xb = rs.rand(80_000, 128).astype(np.float32) + np.linspace(-2, 5, 128, dtype=np.float32)  # per-dimension offsets
    xq = rs.rand(100, 128).astype(np.float32) + np.linspace(-2, 5, 128, dtype=np.float32)
    for metric in (L2, IP):
        cl, ex = _pair(mf, 128, metric, xb)
        _check(cl, ex, xq, 10, metric, xb, oracle_rows=32)
        assert cl.collect_stats()["overflows"] == 0


@pytest.mark.parametrize("seed", range(12))
def test_collect_fuzz(mf, seed):
    rs = np.random.RandomState(9000 + seed)
    d = int(rs.choice([65, 96, 100, 127, 128]))
    n = int(rs.choice([4096, 5000, 8191, 20000, 33333, 70001]))
    nq = int(rs.choice([20, 21, 64, 255, 513, 600]))
    k = int(rs.choice([1, 2, 7, 10, 11, 15]))
    metric = [L2, IP][rs.randint(2)]
    idmap = bool(rs.randint(2))
    scale = float(rs.choice([1.0, 1e-3, 300.0]))
    xb = ((rs.rand(n, d).astype(np.float32) - (0.5 if rs.randint(2) else 0.0)) * scale).astype(np.float32)
    xq = ((rs.rand(nq, d).astype(np.float32) - 0.5) * scale).astype(np.float32)
    if rs.randint(2):
        xb[rs.randint(0, n, n // 10)] = xb[rs.randint(0, n, n // 10)]
        xq[: nq // 4] = xb[rs.randint(0, n, nq // 4)]
    ids = (rs.permutation(3 * n)[:n] + 5).astype(np.int64) if idmap else None
    desc = "IDMap,Flat" if idmap else "Flat"
    cl, ex = _pair(mf, d, metric, xb, desc=desc, ids=ids)
    D1, I1 = cl.search(xq, k)
    assert cl.last_kernel_info()["name"] == KERNEL
    D0, I0 = ex.search(xq, k)
    what = f"seed={seed} d={d} n={n} nq={nq} k={k} metric={metric} idmap={idmap} scale={scale}"
    assert np.array_equal(I1, I0), what
    assert np.array_equal(D1.view(np.uint32), D0.view(np.uint32)), what
    o = orc.Index(d, desc, metric)
    o.add_with_ids(xb, ids) if idmap else o.add(xb)
    Do, Io = o.search(xq, k)
    assert np.array_equal(I1, Io) and np.array_equal(D1.view(np.uint32), Do.view(np.uint32)), what


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("idmap", [False, True])
@pytest.mark.parametrize("frac,d,k", [(0.3, 128, 10), (0.02, 128, 10), (0.2, 128, 24), (0.4, 48, 10)])  # (k = 24: 32 row classes; d = 48: padded rows)
def test_selector_searches_on_the_coarse_filter(mf, metric, idmap, frac, d, k):
    """filtered search (IDSelectorBitmap / IDSelectorBatch, the reference's signature feature): the selector becomes one bit per
    row, rejected rows are neither candidates nor evidence for the bound, candidates are re-scored with the per-pair
    arithmetic FAISS uses under a selector; must equal the exact kernels' SEL instances and the oracle bit for bit"""
    from helpers import bitmap_from_ids

    rs = np.random.RandomState(17 + int(frac * 100))
    n, nq = 150_000, 300
    xb = rs.rand(n, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xq = rs.rand(nq, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xb[rs.randint(0, n, 2000)] = xb[rs.randint(0, n, 2000)]
    ids = (rs.permutation(4 * n)[:n] + 3).astype(np.int64) if idmap else np.arange(n, dtype=np.int64)
    desc = "IDMap,Flat" if idmap else "Flat"
    cl, ex = _pair(mf, d, metric, xb, desc=desc, ids=ids if idmap else None)
    o = orc.Index(d, desc, metric)
    o.add_with_ids(xb, ids) if idmap else o.add(xb)
    keep = ids[rs.rand(n) < frac]
    for sel in (("batch", keep), ("bitmap", bitmap_from_ids(ids, np.isin(ids, keep)))):
        D1, I1 = cl.search(xq, k, sel=sel)
        assert cl.last_kernel_info()["name"] == KERNEL
        D0, I0 = ex.search(xq, k, sel=sel)
        assert ex.last_kernel_info()["name"] != KERNEL
        assert np.isin(I1[I1 >= 0], keep).all()
        assert np.array_equal(I1, I0) and np.array_equal(D1.view(np.uint32), D0.view(np.uint32)), (metric, idmap, sel[0])
        Do, Io = o.search(xq[:64], k, sel=sel)
        assert np.array_equal(I1[:64], Io) and np.array_equal(D1[:64].view(np.uint32), Do.view(np.uint32))


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", [1, 3, 8, 13, 19])
def test_small_batches_take_faiss_per_pair_branch_on_the_coarse_filter(mf, metric, nq):
    """fewer than 20 queries: FAISS computes sum (x_k - y_k)^2 per pair (not the norms formula); from 8 queries on a large
    database the coarse filter serves these too (a single query included) and re-scores in that arithmetic, also for the queries it re-runs"""
    rs = np.random.RandomState(100 + nq)
    d, n, k = 128, 300_000, 10
    xb = rs.rand(n, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xq = rs.rand(nq, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xb[rs.randint(0, n, 3000)] = xb[rs.randint(0, n, 3000)]
    xq[0] = xb[7]
    if nq > 2:
        xq[2, 5] = np.nan  # re-run on the exact kernels, in the same branch's arithmetic
    ix = mf.index_factory(d, "Flat", metric)
    ix.add(xb)
    D, I = ix.search(xq, k)
    assert ix.last_kernel_info()["name"] == KERNEL
    Do, Io = orc.flat_search(metric, xb, xq, k)  # PATH_AUTO: the per-pair branch for nq < 20
    assert np.array_equal(I, Io) and np.array_equal(D.view(np.uint32), Do.view(np.uint32))
    ix.set_option("prefilter", 0)
    D0, I0 = ix.search(xq, k)
    assert ix.last_kernel_info()["name"] != KERNEL
    assert np.array_equal(I, I0) and np.array_equal(D.view(np.uint32), D0.view(np.uint32))


@pytest.mark.parametrize("with_sel", [False, True])
def test_inner_product_ties_are_resolved_from_the_candidate_list(mf, with_sel):
    """A tie crossing rank k (integer data: dozens of rows share the k-th score) is FAISS's heap outcome.  The
    rows at or above the boundary score all are candidates of the coarse filter, so the outcome is computed from that list --
    no second pass over the database; it must equal the re-scan (option tie_from_candidates = 0) and the oracle."""
    rs = np.random.RandomState(31)
    xb = rs.randint(-2, 3, size=(90_000, 96)).astype(np.float32)
    xq = rs.randint(-2, 3, size=(300, 96)).astype(np.float32)
    sel = ("batch", np.sort(rs.permutation(90_000)[:60_000]).astype(np.int64)) if with_sel else None
    cl, ex = _pair(mf, 96, IP, xb)
    D1, I1 = cl.search(xq, 7, sel=sel)
    assert cl.last_kernel_info()["name"] == KERNEL
    cl.set_option("tie_from_candidates", 0)
    D2, I2 = cl.search(xq, 7, sel=sel)
    D0, I0 = ex.search(xq, 7, sel=sel)
    o = orc.Index(96, "Flat", IP)
    o.add(xb)
    Do, Io = o.search(xq, 7, sel=sel)
    assert (Do[:, 6] == Do[:, 5]).mean() > 0.25  # (the data does tie around rank k)
    for D, I in ((D1, I1), (D2, I2), (D0, I0)):
        assert np.array_equal(I, Io) and np.array_equal(D, Do)


@pytest.mark.parametrize("metric", [L2, IP])
def test_stream_overflow_takes_out_only_the_heavy_queries(mf, metric):
    """a few queries sit on a vector stored tens of thousands of times (every copy is a candidate,
    rightly); the stream overflows by far more than growing it would cure.  Only those queries leave the coarse filter (they are
    re-run on the exact kernel), the scan runs once more for the others -- the batch stays on flat_bf16_collect_kernel and every
    answer is the exact kernel's and the oracle's."""
    rs = np.random.RandomState(17)
    d, nb, nq = 128, 150_000, 600
    xb = rs.rand(nb, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    hot = rs.rand(d).astype(np.float32) - (0.5 if metric == IP else 0.0)  # (a vector like any other: only queries ON it are hot)
    xb[rs.permutation(nb)[:60_000]] = hot  # 60 000 copies of one vector
    xq = rs.rand(nq, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xq[[5, 77, 300, 411, 599]] = hot
    cl, ex = _pair(mf, d, metric, xb)
    cl.set_option("cl_stream_cap", 128)  # 128 entries per query: the five hot queries alone hold 300 000
    D1, I1 = _check(cl, ex, xq, 10, metric, xb, oracle_rows=100)
    st, pf = cl.collect_stats(), cl.prefilter_stats()
    assert st["overflows"] == 1 and st["queries"] == nq, st  # one overflow, then the second scan served the batch
    assert 5 <= pf["fallback_queries"] <= 40, pf  # the hot queries (and hardly anybody else) went to the exact kernel
    cl.set_option("cl_stream_cap", 0)


def test_stream_overflow_grows_the_stream_for_data_that_needs_it(mf):
    """clustered rows with large norms admit thousands of rows per query (tools/collect_sensitivity.py): the stream is grown
    once, the scan repeated, and the index remembers the size"""
    xb = orc.synth_clustered(200_000, 128, 5, n_centers=64, sigma=0.1)
    xq = orc.synth_clustered(700, 128, 6, n_centers=64, sigma=0.1)
    cl, ex = _pair(mf, 128, L2, xb)
    cl.set_option("cl_stream_cap", 1024)  # (whole clusters of ~3 000 rows are within the bound of their queries)
    _check(cl, ex, xq, 10, L2, xb, oracle_rows=64)
    st = cl.collect_stats()
    assert st["overflows"] == 1 and st["queries"] == 700 and st["candidates"] > 700 * 1024, st
    assert cl.prefilter_stats()["fallback_queries"] == 0
    cl.set_option("cl_stream_cap", 0)


@pytest.mark.parametrize("metric", [L2, IP])
def test_round4_switches_do_not_change_a_single_bit(mf, metric):
    """Round 4 changed HOW the scan gets its bounds and how the candidates reach the re-scoring, not what comes out: the error bound
    from the actual rounding residuals (cl_bound_mode), the pass bounds through the global table (cl_tab), the candidate count kept on
    the device (cl_defer_count) -- every combination returns the labels and distances of the exact f32 kernel, searched twice so that
    the second search of an index (sort sized from the first one's candidate count) is covered, also after rows were added."""
    rs = np.random.RandomState(41)
    d, nb, nq, k = 128, 140_000, 700, 10
    xb = rs.rand(nb + 30_000, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xb[::97] = xb[5]
    xq = rs.rand(nq, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    ex = mf.index_factory(d, "Flat", metric)
    ex.set_option("prefilter", 0)
    ex.add(xb[:nb])
    D0, I0 = ex.search(xq, k)
    ex.add(xb[nb:])
    D0b, I0b = ex.search(xq, k)
    cands = {}
    try:
        for bound in (1, 0):
            for tab in (1, 0):
                for defer in (1, 0):
                    cl = mf.index_factory(d, "Flat", metric)
                    cl.set_option("prefilter", 2)
                    cl.set_option("cl_bound_mode", bound)
                    cl.set_option("cl_tab", tab)
                    cl.set_option("cl_defer_count", defer)
                    cl.add(xb[:nb])
                    for rep in range(2):
                        D, I = cl.search(xq, k)
                        assert cl.last_kernel_info()["name"] == KERNEL
                        assert np.array_equal(I, I0) and np.array_equal(D.view(np.uint32), D0.view(np.uint32)), (bound, tab, defer, rep)
                    cl.add(xb[nb:])  # more rows than the previous search's estimate was made for
                    D, I = cl.search(xq, k)
                    assert np.array_equal(I, I0b) and np.array_equal(D.view(np.uint32), D0b.view(np.uint32)), (bound, tab, defer, "added")
                    st = cl.collect_stats()
                    cands[(bound, tab)] = st["candidates"] / st["queries"]
    finally:
        cl = mf.index_factory(d, "Flat", metric)
        cl.set_option("cl_bound_mode", 1)  # (process-wide knobs back to their defaults)
        cl.set_option("cl_tab", 1)
    assert cands[(1, 1)] < 0.8 * cands[(0, 1)], cands  # the residual-norm bound admits clearly fewer rows


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_sort_sized_too_small_is_run_again(mf, metric):
    """cl_est: 'the previous search of this index had v candidates per query'.  1 -> the deferred sort covers far too few entries,
    the search notices at its one synchronisation and runs again the synchronous way; 100 000 -> far too many (capped by the
    stream); both return the exact kernel's bits.  Also a batch whose heaviest queries hold more than 1 024 candidates (duplicated
    rows): collect_select_kernel's chunked path."""
    rs = np.random.RandomState(77)
    d, nb, nq, k = 128, 90_000, 300, 10
    xb = rs.rand(nb, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xb[1000:3500] = xb[7]  # 2 500 copies of one row: every query near it holds all of them
    xq = rs.rand(nq, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xq[:40] = xb[7] + 1e-3 * rs.rand(40, d).astype(np.float32)
    ex = mf.index_factory(d, "Flat", metric)
    ex.set_option("prefilter", 0)
    ex.add(xb)
    D0, I0 = ex.search(xq, k)
    cl = mf.index_factory(d, "Flat", metric)
    cl.set_option("prefilter", 2)
    cl.add(xb)
    for est in (0, 1, 100000, 0):
        if est:
            cl.set_option("cl_est", est)
        D, I = cl.search(xq, k)
        assert cl.last_kernel_info()["name"] == KERNEL
        assert np.array_equal(I, I0) and np.array_equal(D.view(np.uint32), D0.view(np.uint32)), est


@pytest.mark.gpu
@pytest.mark.parametrize("d,k", [(128, 16), (128, 32), (128, 127), (768, 32), (256, 16)])
def test_inner_product_filter_works_with_the_users_k(mf, d, k):
    """Inner product carries k + 1 entries for the tie detection; the FILTER works with k (a row tied with the k-th score passes any
    bound derived from k rows), so k = 32 stays on the coarse filter of the wide stores and on the 32-class instance at d <= 128.
    Small-integer data with duplicated rows: ties at the k-th score in most queries; equal to the exact kernels (FAISS's heap)."""
    rs = np.random.RandomState(100 + d + k)
    nb, nq = 70_000, 200
    xb = rs.randint(-2, 3, size=(nb, d)).astype(np.float32)
    m = nb // 3
    xb[0 : 3 * m : 3] = xb[1 : 3 * m : 3]
    xq = rs.randint(-2, 3, size=(nq, d)).astype(np.float32)
    ex = mf.index_factory(d, "Flat", IP)
    ex.set_option("prefilter", 0)
    ex.add(xb)
    D0, I0 = ex.search(xq, k)
    cl = mf.index_factory(d, "Flat", IP)
    cl.set_option("prefilter", 2)
    cl.add(xb)
    D, I = cl.search(xq, k)
    assert "bf16" in cl.last_kernel_info()["name"] and "x3" not in cl.last_kernel_info()["name"], cl.last_kernel_info()["name"]
    assert np.array_equal(I, I0) and np.array_equal(D.view(np.uint32), D0.view(np.uint32))


@pytest.mark.parametrize("case", ["plain", "idmap", "selector", "few_queries", "duplicates", "k64"])
def test_bucketed_finish_of_the_l2_filter_equals_the_sorted_pipeline(mf, case):
    """round 5, option cl_fbucket (d = 128, L2): final-bound filter -> per-query row buckets -> one wavefront per query re-scores and
    one selects (csrc/ivf_collect.hip, shared with the IVF path) instead of radix sort -> segments -> re-scoring -> selection ->
    emission.  Same labels, same distance bits as the sorted pipeline, the exact f32 kernel and the oracle; a bucket too small for
    the data (option cl_fpitch) is grown and the finish repeated; beyond 16 384 entries per query the sorted pipeline takes the index back."""
    rs = np.random.RandomState(17)
    d, nb, nq, k = 128, 120_000, (13 if case == "few_queries" else 500), (64 if case == "k64" else 10)
    xb = rs.rand(nb, d).astype(np.float32)
    if case == "duplicates":
        xb[nb // 2 :: 3] = xb[: len(xb[nb // 2 :: 3])]
    xq = rs.rand(nq, d).astype(np.float32)
    xq[: nq // 5] = xb[11 : 11 + nq // 5]
    ids = np.arange(nb, dtype=np.int64) * 7 + 3 if case == "idmap" else None
    cl, ex = _pair(mf, d, L2, xb, "IDMap,Flat" if case == "idmap" else "Flat", ids)
    sel = None
    if case == "selector":
        keep = np.arange(nb, dtype=np.int64)[::3]
        sel = ("batch", keep)
    c0 = cl.collect_stats()
    D1, I1 = cl.search(xq, k, sel=sel)
    assert cl.last_kernel_info()["name"] == KERNEL
    c1, adm = cl.collect_stats(), cl.ivf_probe_stats()["admitted"]
    # (collect_stats counts what the exact stage re-scored: the survivors of the final-bound filter, never more than the scan admitted)
    assert c1["queries"] - c0["queries"] == nq and 0 < c1["candidates"] - c0["candidates"] <= adm, (c0, c1, adm)
    cl.set_option("cl_fbucket", 0)
    D0, I0 = cl.search(xq, k, sel=sel)
    assert cl.last_kernel_info()["name"] == KERNEL
    De, Ie = ex.search(xq, k, sel=sel)
    assert np.array_equal(I1, I0) and np.array_equal(D1.view(np.uint32), D0.view(np.uint32)), "bucketed finish differs from the sorted pipeline"
    assert np.array_equal(I1, Ie) and np.array_equal(D1.view(np.uint32), De.view(np.uint32)), "differs from the exact f32 kernel"
    if case in ("plain", "duplicates", "few_queries"):
        Do, Io = orc.flat_search(L2, xb, xq[:64], k, force_path=orc.PATH_BLAS if nq >= 20 else orc.PATH_PAIR)
        assert np.array_equal(I1[:64], Io[: len(I1[:64])]) and np.array_equal(D1[:64].view(np.uint32), Do[: len(D1[:64])].view(np.uint32))
    if case == "duplicates":  # a 64-entry bucket overflows on a query that sits on many copies: the pitch grows, the finish runs again, same bits
        xb2 = np.tile(xb[:64], (2000, 1))
        c2, e2 = _pair(mf, d, L2, xb2)
        c2.set_option("cl_fbucket", 1)
        c2.set_option("cl_fpitch", 64)
        D2, I2 = c2.search(xb2[:300].copy(), k)
        D3, I3 = e2.search(xb2[:300].copy(), k)
        assert np.array_equal(I2, I3) and np.array_equal(D2.view(np.uint32), D3.view(np.uint32))


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [128, 768])
def test_outlier_rows_stay_out_of_the_store_and_in_every_candidate_set(mf, metric, d):
    """round 6: the coarse filter's E scales with the LARGEST ||y - mu|| of the store -- one row of 100 x the usual norm
    made every query admit thousands of rows (17.5 -> 602 ms per batch at the headline).  Rows beyond 64 x the mean squared centred norm
    are kept out of the bf16 store and appended to every query's candidates: same answers as the exact kernel and the oracle -- also for
    queries whose nearest row IS an outlier -- and the candidate count stays what it is without them."""
    rs = np.random.RandomState(1000 + d + metric)
    nb, nq, k = 270_000, 300, 10
    xb = rs.randn(nb, d).astype(np.float32)
    xq = rs.randn(nq, d).astype(np.float32)
    plain, ex0 = _pair(mf, d, metric, xb)
    plain.search(xq, k)
    base = plain.collect_stats()["candidates"] / nq
    out_rows = [12345, 200_001, 269_999]
    xb2 = xb.copy()
    xb2[out_rows] *= 100.0
    xq2 = xq.copy()
    xq2[:3] = xb2[out_rows] * 1.001  # queries that sit on the outliers: under L2 their nearest row is the outlier itself
    cl, ex = _pair(mf, d, metric, xb2)
    D, I = cl.search(xq2, k)
    assert cl.last_kernel_info()["name"] == (KERNEL if d <= 128 else "flat_bf16_big_kernel")
    D0, I0 = ex.search(xq2, k)
    assert np.array_equal(I, I0) and np.array_equal(D.view(np.uint32), D0.view(np.uint32)), "differs from the exact f32 kernel"
    Do, Io = orc.flat_search(metric, xb2, xq2[:32], k, force_path=orc.PATH_BLAS)
    assert np.array_equal(I[:32], Io) and np.array_equal(D[:32].view(np.uint32), Do.view(np.uint32)), "differs from the oracle"
    assert cl.get_stat("flat_outlier_rows") == 3
    if metric == L2:
        assert [int(I[j][0]) for j in range(3)] == out_rows
    else:  # inner product: the outliers' huge norms put them on top for every query with a positive score
        assert set(out_rows) & set(I[:, 0].tolist())
    per_query = cl.collect_stats()["candidates"] / nq
    assert per_query < 2.0 * base + 3 + 5, (per_query, base)  # (3 appended rows per query; without the handling: thousands)
    # switched off: still exact (the stream grows or the fall-back takes the batch), only slower
    off = mf.index_factory(d, "Flat", metric)
    off.set_option("prefilter", 2)
    off.set_option("outlier_rows", 0)
    for i0 in range(0, nb, 1 << 16):
        off.add(xb2[i0 : i0 + (1 << 16)])
    D0, I0 = off.search(xq2, k)
    assert off.get_stat("flat_outlier_rows") == 0
    assert np.array_equal(I0, I) and np.array_equal(D0.view(np.uint32), D.view(np.uint32))


def _nonfinite(xq):
    xq[3, 1] = np.nan  # no finite bound for these two: the filter hands them to rerun_unproven
    xq[4] *= 1e19
    return xq


@pytest.mark.parametrize("metric", [L2, IP])
def test_rerun_inside_the_per_pair_branch_inherits_the_branch_and_leaves_no_trace(mf, metric):
    """fewer than 20 queries, two of them re-run: the re-run is a request of its own that inherits FAISS's per-pair branch from its batch
    (two queries alone would not say), and it is quiet -- the search's dominant kernel stays the filter's"""
    rs = np.random.RandomState(640 + metric)
    d, nb, nq, k = 64, 66_000, 16, 5
    xb = rs.rand(nb, d).astype(np.float32) - (0.5 if metric == IP else 0.0)
    xq = _nonfinite(rs.rand(nq, d).astype(np.float32) - (0.5 if metric == IP else 0.0))
    cl, ex = _pair(mf, d, metric, xb)
    D1, I1 = cl.search(xq, k)
    name, fb = cl.last_kernel_info()["name"], cl.prefilter_stats()["fallback_queries"]
    print("pair-branch re-run: metric", metric, "kernel", name, "fallback_queries", fb)
    D0, I0 = ex.search(xq, k)
    assert np.array_equal(I1, I0) and np.array_equal(D1.view(np.uint32), D0.view(np.uint32)), "differs from prefilter = 0"
    Do, Io = orc.flat_search(metric, xb, xq, k, force_path=orc.PATH_PAIR)
    assert np.array_equal(I1, Io) and np.array_equal(D1.view(np.uint32), Do.view(np.uint32)), "differs from the oracle's per-pair path"
    assert 1 <= fb <= 2
    assert name == KERNEL  # (the quiet re-run left no trace)


@pytest.mark.parametrize("desc", ["Flat", "IDMap,Flat"])
def test_rerun_under_the_tie_wrapper_in_the_blas_branch(mf, desc):
    """inner product over small integers (ties at the k-th score everywhere), two queries re-run: the re-run passes the tie wrapper for
    its own queries after the batch's flags have been consumed"""
    rs = np.random.RandomState(9)
    d, nb, nq, k = 32, 70_000, 64, 10
    xb = rs.randint(-3, 4, size=(nb, d)).astype(np.float32)
    xq = _nonfinite(rs.randint(-3, 4, size=(nq, d)).astype(np.float32))
    ids = (rs.permutation(400_000)[:nb] + 11).astype(np.int64) if desc != "Flat" else None
    cl, ex = _pair(mf, d, IP, xb, desc=desc, ids=ids)
    D1, I1 = cl.search(xq, k)
    fb = cl.prefilter_stats()["fallback_queries"]
    print("tie-wrapper re-run:", desc, "kernel", cl.last_kernel_info()["name"], "fallback_queries", fb)
    D0, I0 = ex.search(xq, k)
    assert np.array_equal(I1, I0) and np.array_equal(D1.view(np.uint32), D0.view(np.uint32)), "differs from prefilter = 0"
    if ids is None:
        Do, Io = orc.flat_search(IP, xb, xq, k, force_path=orc.PATH_BLAS)
    else:
        o = orc.Index(d, desc, IP)
        o.add_with_ids(xb, ids)
        Do, Io = o.search(xq, k)  # (64 queries: the BLAS branch)
    fin = np.isfinite(xq).all(axis=1) & (np.abs(xq).max(axis=1) < 1e18)
    assert fin.sum() == nq - 2
    assert np.array_equal(I1[fin], Io[fin]) and np.array_equal(D1[fin].view(np.uint32), Do[fin].view(np.uint32)), "differs from the oracle"
    assert fb >= 2


@pytest.mark.parametrize("prefilter", [None, 2])
def test_small_inner_product_batch_asks_the_filter_twice_with_the_same_outcome(mf, prefilter):
    """inner product, 8..19 queries, no selector: the route asks the coarse filter before it settles on the MFMA kernel and again after
    (DESIGN.md 3.1); kernel and statistics are what they were before the route was written as one chain"""
    rs = np.random.RandomState(12)
    d, nb, nq, k = 64, 66_000, 12, 5
    xb = rs.rand(nb, d).astype(np.float32) - 0.5
    xq = rs.rand(nq, d).astype(np.float32) - 0.5
    ix, ex = mf.index_factory(d, "Flat", IP), mf.index_factory(d, "Flat", IP)
    if prefilter is not None:
        ix.set_option("prefilter", prefilter)
    ex.set_option("prefilter", 0)
    ix.add(xb), ex.add(xb)
    D1, I1 = ix.search(xq, k)
    name = ix.last_kernel_info()["name"]
    print("twice-asked filter: prefilter", prefilter, "kernel", name, "prefilter_stats", ix.prefilter_stats(), "collect_stats", ix.collect_stats())
    D0, I0 = ex.search(xq, k)
    assert np.array_equal(I1, I0) and np.array_equal(D1.view(np.uint32), D0.view(np.uint32)), "differs from prefilter = 0"
    Do, Io = orc.flat_search(IP, xb, xq, k, force_path=orc.PATH_PAIR)
    assert np.array_equal(I1, Io) and np.array_equal(D1.view(np.uint32), Do.view(np.uint32)), "differs from the oracle's per-pair path"
    assert name == ("flat_mfma_kernel" if prefilter is None else KERNEL)
