"""IndexIVFPQFastScan on the device against the numpy float32 model of its contract (tests/ivfpqfs_reference.py).  Centroids, codebooks,
rows and queries are small integers, so labels and distance bits are compared for equality."""
import numpy as np
import pytest

import ivfpqfs_reference as ref
from helpers import bitmap_from_ids

pytestmark = pytest.mark.gpu

L2, IP = ref.L2, ref.IP
NLIST = 8
# equal norms, so that a row c + r lands on c under both metrics for |r| small against the gaps (the first two components; the rest are 0)
DIRS = 16 * np.array([(7, 1), (5, 5), (1, 7), (-1, 7), (-5, 5), (-7, 1), (-7, -1), (-5, -5)], dtype=np.float32)
NQS, KS = (1, 16, 17, 130), (1, 10, 2048)
CASES = [(2, 1), (6, 2), (8, 1), (34, 2), (66, 1)]  # (M, dsub): one step, a partial K-group, two steps, past one dword plane, SMAX = 32


def _mf():
    import mi355_faiss as mf

    return mf


def _data(M, dsub, sizes, seed=0):
    """-> centroids, codebooks (distinct values per (m, j) in every component), rows planted on the centroids by list size, queries"""
    rng = np.random.default_rng(1000 * M + 10 * dsub + seed)
    d = M * dsub
    cent = np.zeros((NLIST, d), dtype=np.float32)
    cent[:, :2] = DIRS
    cb = np.stack([np.stack([rng.permutation(16) for _ in range(dsub)], axis=1) + m % 5 for m in range(M)]).astype(np.float32)
    of = rng.permutation(np.repeat(np.arange(NLIST), sizes))
    xb = cent[of] + rng.integers(-4, 12, (of.size, d)).astype(np.float32)
    xq = cent[rng.integers(0, NLIST, NQS[-1])] + rng.integers(-4, 12, (NQS[-1], d)).astype(np.float32)
    return cent, cb, xb, xq


def _index(metric, cent, cb, xb=None, ids=None):
    mf = _mf()
    M, _, dsub = cb.shape
    ix = mf.IndexIVFPQFastScan(M * dsub, NLIST, M, 4, metric)
    assert ix.kind == mf.KIND_IVFPQFS and not ix.is_trained
    ix.ivf_set_centroids(cent)
    ix.pq_set_centroids(cb)
    assert ix.is_trained and ix.pq_info() == (M, 4)
    if xb is not None:
        ix.add(xb) if ids is None else ix.add_with_ids(xb, ids)
    return ix


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: labels differ in {(got[1] != want[1]).sum()} slots"
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"{what}: distances differ in {(got[0] != want[0]).sum()} slots"


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("M,dsub", CASES)
def test_search_equals_the_model(M, dsub, metric):
    probe = _index(metric, *_data(M, dsub, [1] * NLIST)[:2])
    R, Q = probe.get_stat("ivfpqfs_rows_per_workgroup"), probe.get_stat("ivfpqfs_pair_block")
    assert Q == {2: 128, 6: 128, 8: 128, 34: 64, 66: 32}[M] and NQS[-1] > Q
    sizes = [R + 40, 0, 1, 15, 16, 17, 33, 5]  # a list past one segment and one bucket; an empty one; around one row tile
    cent, cb, xb, xq = _data(M, dsub, sizes)
    ix = _index(metric, cent, cb, xb)
    lists = ref.build_lists(metric, cent, cb, xb)
    for l in range(NLIST):
        ids, codes = ix.ivfpq_list(l)
        assert ids.size == sizes[l] and np.array_equal(ids, lists[l][0]) and np.array_equal(codes, ref.pack(lists[l][1])), f"list {l}"
    dis = ref.all_pair_distances(metric, cent, cb, lists, xq)
    for nprobe in (1, 3, NLIST + 3):  # (nprobe > nlist: every list, each by nq pairs -- 1, 16, 17 and more than Q)
        want = ref.search(metric, cent, cb, lists, dis, xq, KS[-1], nprobe)  # a query's list is a prefix of its longest, alone or in a batch
        for nq in NQS:
            for k in KS:
                _same(ix.search(xq[:nq], k, nprobe=nprobe), (want[0][:nq, :k], want[1][:nq, :k]), f"nprobe {nprobe} nq {nq} k {k}")
    assert ix.last_kernel_info()["name"] == "ivfpqfs_scan_kernel" and ix.get_stat("ivfpqfs_scan_rescans") > 0


@pytest.mark.parametrize("metric", [L2, IP])
def test_ties_selectors_ids_zero_span_and_non_finite_queries(metric):
    cent, cb, xb, xq = _data(6, 2, [3, 2, 0, 4, 1, 2, 2, 3])
    xb = np.tile(xb, (40, 1))  # every row 40 times in its list: ties fall to probe rank, then position
    ids = np.arange(xb.shape[0], dtype=np.int64)[::-1] * 3 + 1
    ix = _index(metric, cent, cb, xb, ids)
    lists = ref.build_lists(metric, cent, cb, xb, ids)
    xq = xq[:17].copy()
    xq[3, 4], xq[9, 0] = np.inf, np.nan  # no valid pair: only missing slots
    dis = ref.all_pair_distances(metric, cent, cb, lists, xq)
    got = ix.search(xq, 50, nprobe=NLIST)
    _same(got, ref.search(metric, cent, cb, lists, dis, xq, 50, NLIST), "duplicated rows, add_with_ids")
    assert (got[1][[3, 9]] == -1).all() and (np.diff(got[0][0]) == 0).any()
    for q in (0, 16):
        _same(ix.search(xq[q : q + 1], 50, nprobe=NLIST), (got[0][q : q + 1], got[1][q : q + 1]), f"query {q} alone")
    keep = ids % 3 != 2
    keep[::5] = False
    want = ref.search(metric, cent, cb, lists, dis, xq, 10, 4, keep_ids=ids[keep])
    _same(ix.search(xq, 10, nprobe=4, sel=("bitmap", bitmap_from_ids(ids, keep))), want, "bitmap")
    _same(ix.search(xq, 10, nprobe=4, sel=("program", [(_mf().SELOP_ARRAY, ids[keep], 0, 0)])), want, "selector program")
    flat = np.repeat(cb[:, :1], 16, axis=1)  # all-equal codebooks: span == 0, every score 0, a pair's distance is its b
    iz = _index(metric, cent, flat, xb)
    lz = ref.build_lists(metric, cent, flat, xb)
    _same(iz.search(xq, 30, nprobe=NLIST), ref.search(metric, cent, flat, lz, ref.all_pair_distances(metric, cent, flat, lz, xq), xq, 30, NLIST), "span == 0")


def test_remove_merge_clone_reconstruct_and_refusals(tmp_path):
    mf = _mf()
    cent, cb, xb, xq = _data(8, 2, [40, 0, 7, 16, 17, 30, 9, 21])
    n, half = xb.shape[0], xb.shape[0] // 2
    ix, other = _index(L2, cent, cb, xb[:half]), _index(L2, cent, cb, xb[half:])
    ix.merge_from(other, add_id=half)
    assert ix.ntotal == n and other.ntotal == 0
    xq = xq[:17]
    lists = ref.build_lists(L2, cent, cb, xb)
    _same(ix.search(xq, 10, nprobe=3), ref.search(L2, cent, cb, lists, ref.all_pair_distances(L2, cent, cb, lists, xq), xq, 10, 3), "the joined rows")
    gone = np.arange(0, n, 3, dtype=np.int64)
    assert ix.remove_ids(("batch", gone)) == gone.size
    left = np.setdiff1d(np.arange(n), gone)
    of_row, _ = ref.ivr.assign(L2, cent, xb)
    codes = ref.encode(cb, ref.ivr.residuals(cent, xb, of_row))
    lists = []  # (removal reorders a list as FAISS does: the model takes every list's order from the device, its rows must be the survivors)
    for l in range(NLIST):
        ids, packed = ix.ivfpq_list(l)
        assert np.array_equal(np.sort(ids), left[of_row[left] == l]) and np.array_equal(packed, ref.pack(codes[ids])), f"list {l}"
        lists.append((ids, codes[ids]))
    want = ref.search(L2, cent, cb, lists, ref.all_pair_distances(L2, cent, cb, lists, xq), xq, 10, 3)
    for probe in (ix, ix.clone_to_gpu(0)):
        assert probe.kind == mf.KIND_IVFPQFS
        _same(probe.search(xq, 10, nprobe=3), want, "the surviving rows, cloned")
    rec = cent[of_row] + ref.decode(cb, codes)
    assert np.array_equal(ix.reconstruct_batch(left[[5, 0, 5]]), rec[left[[5, 0, 5]]]) and np.array_equal(ix.reconstruct(int(left[-1])), rec[left[-1]])
    for call in (lambda: mf.write_index(ix, str(tmp_path / "x.index")), lambda: ix.range_search(xq[:2], 5.0), lambda: mf.IndexIVFPQFastScan(16, 4, 8, 8),
                 lambda: mf.IndexIVFPQFastScan(21, 4, 7), lambda: mf.IndexIVFPQFastScan(260, 4, 130), lambda: mf.index_factory(16, "IVF8,PQ4x4fs", L2)):
        with pytest.raises(mf.FaissException, match="This index type is not implemented on the MI355X path yet: "):
            call()
    with pytest.raises(mf.FaissException, match="multiple of the number of subquantizers"):
        mf.IndexIVFPQFastScan(18, 4, 4)
    with pytest.raises(mf.FaissException, match="unknown option"):
        ix.set_option("ivfpq_precomputed_table", 1)
    with pytest.raises(mf.FaissException, match="This index type is not implemented"):
        ix.clone_to_gpu(-1)
