"""Flat L2 on rows that CLUSTER (round 5): the index keeps an IVF index of its rows as a shadow (csrc/index.hip
FlatIndex::shadow_search) -- per-list centring in the coarse filter, the Flat arithmetic in the re-scoring, and a proof per query
that the unprobed lists cannot hold a better row.  The answers must be the Flat index's, bit for bit: labels AND distances equal to
the exact f32 kernel and to the oracle (the reference reaches this through Index::search, src/faiss_extension.cpp:631)."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
L2 = orc.METRIC_L2
TIMED_LAUNCHES = 1  # kernel launches one shadow search of test_shadow_rerun_... brackets with events


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss

    return mi355_faiss


def _same(a, b, what):
    assert np.array_equal(a[1], b[1]), what + ": labels"
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), what + ": distances"


def test_clustered_rows_take_the_shadow_and_stay_bit_exact(mf):
    import torch

    d, n, nq, k = 128, 1_048_576, 2048, 10
    dev = torch.device("cuda", 0)
    ix = mf.index_factory(d, "Flat", L2)
    xb = mf.synth_clustered_torch(n, d, 1234, row0=0, n_centers=1024, sigma=0.1, device=dev)
    ix.add_torch(xb)
    xq = mf.synth_clustered_torch(nq, d, 4321, row0=0, n_centers=1024, sigma=0.1, device=dev)
    D0, I0 = ix.search_torch(xq, k)  # the global-centring coarse filter: ~ a cluster's worth of candidates per query -> the shadow is wanted
    torch.cuda.synchronize()
    assert ix.last_kernel_info()["name"].startswith("flat_bf16_collect")
    assert ix.collect_stats()["candidates"] > 600 * nq
    D1, I1 = ix.search_torch(xq, k)  # builds the shadow, answers through it
    torch.cuda.synchronize()
    assert "flat shadow" in ix.last_kernel_info()["name"], ix.last_kernel_info()
    D2, I2 = ix.search_torch(xq, k)
    torch.cuda.synchronize()
    assert "flat shadow" in ix.last_kernel_info()["name"]
    assert torch.equal(I1, I0) and torch.equal(D1.view(torch.int32), D0.view(torch.int32))
    assert torch.equal(I2, I0) and torch.equal(D2.view(torch.int32), D0.view(torch.int32))
    # ... and the oracle on a query sample (BLAS branch: nq >= 20)
    xb_h = orc.synth_clustered(n, d, 1234, n_centers=1024, sigma=0.1)
    xq_h = xq[:256].cpu().numpy()
    _same((D2[:256].cpu().numpy(), I2[:256].cpu().numpy()), orc.flat_search(L2, xb_h, xq_h, k, force_path=orc.PATH_BLAS), "shadow vs oracle")
    # the exact f32 kernel
    ix.set_option("prefilter", 0)
    De, Ie = ix.search_torch(xq[:512].contiguous(), k)
    torch.cuda.synchronize()
    assert ix.last_kernel_info()["name"].startswith("flat_mfma")
    assert torch.equal(Ie, I2[:512]) and torch.equal(De.view(torch.int32), D2[:512].view(torch.int32))


@pytest.mark.parametrize("kind", ["uniform", "dups"])
def test_rows_that_do_not_cluster_give_the_shadow_up_and_stay_exact(mf, kind):
    """Forced on (option flat_shadow = 1) over uniform rows no unprobed list can be excluded: every query is unproven, the batch takes
    the normal path, the shadow is dropped for good.  Clustered rows with many exact duplicates (ties at the k-th distance inside and
    across lists) stay on the shadow and must order ties by row number as the Flat heap does."""
    d, n, nq, k = 64, 300_000, 600, 10
    if kind == "uniform":
        xb = orc.synth_uniform(n, d, 7)
        xq = orc.synth_uniform(nq, d, 8)
    else:
        xb = orc.synth_clustered(n, d, 7, n_centers=256, sigma=0.05)
        xb = np.round(xb * 8) / 8  # a coarse grid: many rows coincide exactly
        xq = xb[np.random.RandomState(3).randint(0, n, nq)].copy()
    ix = mf.index_factory(d, "Flat", L2)
    ix.add(xb)
    ix.set_option("flat_shadow", 1)
    ref = orc.flat_search(L2, xb, xq, k, force_path=orc.PATH_BLAS)
    for rep in range(3):
        got = ix.search(xq, k)
        _same(got, ref, f"{kind} rep {rep}")
    name = ix.last_kernel_info()["name"]
    if kind == "uniform":
        assert "flat shadow" not in name, name
    else:
        assert "flat shadow" in name, name


def test_shadow_is_extended_by_add_instead_of_rebuilt(mf):
    """round 6: rows added after the shadow was built are APPENDED to it at the next large search (one
    k-means per index, not per add/search cycle); the answers stay the Flat index's bit for bit; the stats say what happened."""
    import torch

    d, n0, step, nq, k = 128, 1_048_576, 65_536, 1024, 10
    dev = torch.device("cuda", 0)
    ix = mf.index_factory(d, "Flat", L2)
    ix.set_option("flat_shadow", 1)  # from the first large search on
    xb = mf.synth_clustered_torch(n0 + 3 * step, d, 1234, row0=0, n_centers=1024, sigma=0.1, device=dev)
    xq = mf.synth_clustered_torch(nq, d, 4321, row0=0, n_centers=1024, sigma=0.1, device=dev)
    ix.add_torch(xb[:n0])
    ix.search_torch(xq, k)
    torch.cuda.synchronize()
    st = ix.shadow_stats()
    assert st["state"] >= 0 and st["rows"] == n0 and st["builds"] == 1 and st["extends"] == 0 and st["device_bytes"] > n0 * d * 2, st
    assert st["build_seconds"] > 0
    for i in range(3):  # DuckDB: insert, then query
        ix.add_torch(xb[n0 + i * step : n0 + (i + 1) * step])
        D, I = ix.search_torch(xq, k)
        torch.cuda.synchronize()
        assert "flat shadow" in ix.last_kernel_info()["name"], ix.last_kernel_info()
        st = ix.shadow_stats()
        assert st["builds"] == 1 and st["extends"] == i + 1 and st["rows"] == n0 + (i + 1) * step, st
    assert int(I.max()) >= n0, "rows added after the build must be found"
    ix.set_option("prefilter", 0)
    ix.set_option("flat_shadow", 0)
    De, Ie = ix.search_torch(xq, k)
    torch.cuda.synchronize()
    assert ix.last_kernel_info()["name"].startswith("flat_mfma")
    assert torch.equal(Ie, I) and torch.equal(De.view(torch.int32), D.view(torch.int32))


def test_a_batch_beyond_the_coarse_matrix_is_served_in_pieces_and_keeps_the_shadow(mf):
    """one batch the coarse quantiser's distance matrix does not cover used to drop a just-built shadow for good."""
    import torch

    d, n, k = 64, 262_144, 10
    dev = torch.device("cuda", 0)
    ix = mf.index_factory(d, "Flat", L2)
    ix.set_option("flat_shadow", 1)
    ix.set_option("flat_shadow_nprobe", 64)
    xb = mf.synth_clustered_torch(n, d, 77, row0=0, n_centers=512, sigma=0.1, device=dev)
    ix.add_torch(xb)
    nq = 262_144 + 5_000  # nlist 512: the 512 MB distance matrix covers 262 144 queries -> two pieces
    xq = mf.synth_clustered_torch(nq, d, 78, row0=0, n_centers=512, sigma=0.1, device=dev)
    D, I = ix.search_torch(xq, k)
    torch.cuda.synchronize()
    assert "flat shadow" in ix.last_kernel_info()["name"], ix.last_kernel_info()
    st = ix.shadow_stats()
    assert st["state"] >= 0 and st["rows"] == n and st["queries"] == nq, st
    ix.set_option("prefilter", 0)
    ix.set_option("flat_shadow", 0)
    for q0 in (0, 262_144 - 512, nq - 1024):
        De, Ie = ix.search_torch(xq[q0 : q0 + 1024].contiguous(), k)
        torch.cuda.synchronize()
        assert torch.equal(Ie, I[q0 : q0 + 1024]) and torch.equal(De.view(torch.int32), D[q0 : q0 + 1024].view(torch.int32))


@pytest.mark.parametrize("how", ["forced", "wanted"])
def test_shadow_rerun_of_fewer_than_20_queries_is_padded_and_restores_nothing_wrongly(mf, how):
    """a handful of queries halfway between two clusters cannot be proven: they are re-run as a request of their own, padded to FAISS's
    BLAS-branch batch size, which the coarse filter may take and the shadow may not -- and the index's shadow state is what it was.
    forced: option flat_shadow = 1 on 131 072 rows (the state stays 0, "not wanted yet": only the automatic mode ever sets 1);
    wanted: the automatic mode on 262 144 rows, where the first search's candidate count sets the state to 1 and the re-run must leave it"""
    d, n, nq, k = 32, (131_072 if how == "forced" else 262_144), 256, 10
    xb = orc.synth_clustered(n, d, 51, n_centers=256, sigma=0.1)
    xq = orc.synth_clustered(nq, d, 52, n_centers=256, sigma=0.1)
    cen = orc.synth_clustered(64, d, 53, n_centers=256, sigma=0.0)  # (sigma = 0: each row is its cluster's centre)
    pairs = [(i, i + 1) for i in range(0, 63, 2) if not np.array_equal(cen[i], cen[i + 1])][:5]
    for j, (a, b) in enumerate(pairs):
        xq[17 + 40 * j] = 0.5 * (cen[a] + cen[b])
    ix = mf.index_factory(d, "Flat", L2)
    ix.add(xb)
    ref = orc.flat_search(L2, xb, xq, k, force_path=orc.PATH_BLAS)
    if how == "forced":
        ix.set_option("prefilter", 2)  # (131 072 rows: below the size from which the automatic mode asks a filter for 256 queries)
        ix.set_option("flat_shadow", 1)
    else:
        _same(ix.search(xq, k), ref, "the coarse filter vs oracle")  # (~ a cluster's worth of candidates per query: the shadow is wanted)
        print("shadow re-run:", how, "first search", ix.last_kernel_info()["name"], ix.collect_stats(), ix.shadow_stats())
    state = 0 if how == "forced" else 1
    assert ix.shadow_stats()["state"] == state
    before = ix.shadow_stats()["unproven"]
    for rep in range(2):
        got = ix.search(xq, k)
        st = ix.shadow_stats()
        print("shadow re-run:", how, "rep", rep, "kernel", ix.last_kernel_info()["name"], "shadow_stats", st, "prefilter_stats", ix.prefilter_stats())
        _same(got, ref, f"rep {rep} vs oracle")
        assert "flat shadow" in ix.last_kernel_info()["name"], ix.last_kernel_info()
        assert st["state"] == state, st  # (the re-run restored nothing wrongly)
        assert 1 <= st["unproven"] - before <= 19, st  # (fewer than 20: the re-run is padded)
        before = st["unproven"]
    ix.set_kernel_timing(True)
    got = ix.search(xq, k)
    count = ix.kernel_time_stats()[0]
    print("shadow re-run:", how, "timed launches of one search", count)
    _same(got, ref, "timed search vs oracle")
    assert count == TIMED_LAUNCHES  # (the quiet re-run times nothing: the same count as before the re-run became a request)
    assert ix.shadow_stats()["state"] == state
    ix.set_kernel_timing(False)
    ix.set_option("prefilter", 0)
    ix.set_option("flat_shadow", 0)
    _same(ix.search(xq, k), got, "exact f32 kernel")
    assert ix.last_kernel_info()["name"].startswith("flat_mfma")
