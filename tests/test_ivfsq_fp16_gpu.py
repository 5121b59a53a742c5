"""GpuIndexIVFScalarQuantizer with QT_fp16 (include/mi355_faiss.h "fp16 scalar-quantised inverted lists") against a plain numpy float64
model over np.float16-rounded residuals.  The model follows the contract's rounding points (the f32 chains m_v and <x, c>, one f32
addition, one fmaf); everything the contract leaves to the matrix pipe it computes exactly.  Coarse centroids go in through the setter, so
no test depends on k-means."""
import functools

import numpy as np
import pytest

import mi355_faiss as mf
import sq_reference as sqr
from helpers import bitmap_from_ids
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
F32, F64 = np.float32, np.float64
NOT_IMPL = "This index type is not implemented on the MI355X path yet"


def _same(got, ref, what):
    (D, I), (Dr, Ir) = got, ref
    assert np.array_equal(I, Ir), f"{what}: labels differ in {(I != Ir).sum()} slots, first query {np.argwhere(I != Ir)[0][0]}"
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32)), f"{what}: distances differ in {(D != Dr).sum()} slots"


def _cent(nlist, d):
    """integer centroids 20 from the origin on a circle in the first two dimensions (d = 1: on a line, 40 apart): a row within 3 per
    component of one goes to it under both metrics when d > 1"""
    c = np.zeros((nlist, d), dtype=F32)
    if d == 1:
        c[:, 0] = 40.0 * np.arange(nlist) - 20.0 * (nlist - 1)
        return c
    t = 2.0 * np.pi * np.arange(nlist) / nlist
    c[:, 0], c[:, 1] = np.rint(20.0 * np.cos(t)), np.rint(20.0 * np.sin(t))
    return c


def _chain(a, b):
    """the f32 chain acc = fmaf(a[k], b[k], acc), k ascending from +0, per row: each step is exact in float64 and rounded once"""
    acc = np.zeros(a.shape[0], dtype=F32)
    for k in range(a.shape[1]):
        acc = (a[:, k].astype(F64) * b[:, k].astype(F64) + acc.astype(F64)).astype(F32)
    return acc


def _pair(metric, c, xq, h):
    """-> (dis [nq, n_l], bound B [nq, n_l]) of the queries against one list's fp16 residuals h"""
    h64 = h.astype(F64)
    with np.errstate(all="ignore"):
        if metric == L2:
            v = (xq - c).astype(F32)
            s = v.astype(F64) @ h64.T
            t = (_chain(v, v)[:, None].astype(F64) + (h64 * h64).sum(1).astype(F32).astype(F64)[None]).astype(F32)
            dis = (-2.0 * s + t.astype(F64)).astype(F32)
            dis = np.where(dis < 0, F32(0), dis)
            B = ((np.abs(v.astype(F64))[:, None, :] + np.abs(h64)[None]) ** 2).sum(2)
        else:
            s = xq.astype(F64) @ h64.T
            base = _chain(xq, np.broadcast_to(c, xq.shape))
            dis = (base[:, None].astype(F64) + s.astype(F32).astype(F64)).astype(F32)
            B = (np.abs(xq.astype(F64))[:, None, :] * (np.abs(h64) + np.abs(c.astype(F64)))[None]).sum(2)
    return dis, (xq.shape[1] + 8) * 2.0**-23 * B


class Model:
    def __init__(self, metric, cent, x, ids=None):
        self.metric, self.cent = metric, cent
        ids = np.arange(x.shape[0], dtype=np.int64) if ids is None else ids
        self.of_row, rows = sqr.assign(metric, cent, x)
        with np.errstate(over="ignore"):
            self.h = sqr.residuals(cent, x, self.of_row).astype(np.float16)
        self.lists = [(ids[r], self.h[r]) for r in rows]

    def pairs(self, xq):
        return [_pair(self.metric, self.cent[l], xq, h_l) if i_l.size else (None, None) for l, (i_l, h_l) in enumerate(self.lists)]

    def search(self, xq, k, nprobe, keep_ids=None):
        P = sqr.probes(self.metric, self.cent, xq, nprobe)
        return sqr.ivf_select(self.metric, P, self.lists, [p[0] for p in self.pairs(xq)], k, keep_ids=keep_ids)


def _index(metric, cent, x=None, ids=None):
    ix = mf.GpuIndexIVFScalarQuantizer(cent.shape[1], cent.shape[0], mf.QT_fp16, metric)
    assert not ix.is_trained
    ix.ivf_set_centroids(cent)
    assert ix.is_trained  # there is no range to wait for
    if x is not None:
        ix.add(x) if ids is None else ix.add_with_ids(x, ids)
    return ix


@functools.lru_cache(maxsize=None)
def _int_case(d, metric):
    """six lists of [0, 1, 15, 17, 65, 200] rows (under L2, and under inner product when d > 1); 66 of the 70 queries sit at the busiest
    list: two full pair groups and a partial one.  Values are small enough for every sum to be exact in f32 in any order, also with the
    2^-13 shifts of the second test: sum |v h| < 2048"""
    rng = np.random.default_rng(1000 * d + metric)
    R = 3 if d <= 128 else 1
    cent = _cent(6, d)
    of = np.repeat(np.arange(6), [0, 1, 15, 17, 65, 200])
    of = of[rng.permutation(of.size)]
    x = (cent[of] + rng.integers(-R, R + 1, (of.size, d))).astype(F32)
    xq = (cent[[5] * 66 + [1, 2, 3, 2]] + rng.integers(-R, R + 1, (70, d))).astype(F32)
    shift = (rng.integers(-3, 4, (70, d)) * 2.0**-13).astype(F32)
    model = Model(metric, cent, x)
    if metric == L2 or d > 1:
        assert [i.size for i, _ in model.lists] == [0, 1, 15, 17, 65, 200]
    for a in (cent, x, xq, shift):
        a.setflags(write=False)
    return cent, x, xq, shift, model


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [1, 33, 128, 520])
@pytest.mark.parametrize("shifted", [False, True], ids=["exact_on_integer_data", "the_query_is_not_rounded_to_fp16"])
def test_integer_data(shifted, d, metric):
    """shifted: the queries move by multiples of 2^-13, exact as hi + lo but not in one fp16 -- a kernel that feeds only hi fails"""
    cent, x, xq, shift, model = _int_case(d, metric)
    xs = (xq + shift).astype(F32) if shifted else xq
    assert np.array_equal(xs.astype(F64), xq.astype(F64) + shift.astype(F64) * shifted)  # (exact in f32)
    assert not shifted or d == 1 or (xs.astype(np.float16).astype(F32) != xs).any()
    ix = _index(metric, cent, x)
    got = ix.search(xs, 10, nprobe=3)
    assert ix.last_kernel_info()["name"] == "sqfp16_scan_kernel" and ix.get_stat("sq_pair_block") == (32 if d <= 512 else 16)
    _same(got, model.search(xs, 10, 3), "integer data")


@functools.lru_cache(maxsize=None)
def _edge_case(metric):
    rng = np.random.default_rng(7 + metric)
    d, counts = 16, [8191, 8192, 8193, 16385]
    cent = _cent(4, d)
    of = np.repeat(np.arange(4), counts)
    of = of[rng.permutation(of.size)]
    x = (cent[of] + rng.integers(-3, 4, (of.size, d))).astype(F32)
    xq = (cent[[0, 1, 2, 3, 3]] + rng.integers(-3, 4, (5, d))).astype(F32)
    for l in range(4):  # the last row of every list is query l itself: the best entry sits at the segment's last position
        x[np.nonzero(of == l)[0][-1]] = xq[l]
    model = Model(metric, cent, x)
    assert [i.size for i, _ in model.lists] == counts
    return cent, x, xq, model


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("k", [1, 100])
def test_segment_and_window_edges(k, metric):
    cent, x, xq, model = _edge_case(metric)
    got = _index(metric, cent, x).search(xq, k, nprobe=2)
    _same(got, model.search(xq, k, 2), "lists of 8191 / 8192 / 8193 / 16385 rows")
    if metric == L2:
        assert (got[0][:4, 0] == 0).all()


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [33, 128])
def test_random_data_within_the_derived_bound(d, metric):
    """B = (d + 8) 2^-23 sum_k (|v_k| + |h_k|)^2 under L2, (d + 8) 2^-23 sum_k |x_k| (|h_k| + |c_k|) under inner product: each f32
    accumulation of d terms (s, m_v or <x, c>, n_h) errs by at most d 2^-24 of the sum of its terms' magnitudes, all of which the
    sum in B dominates; the (hi, lo) split leaves 2^-22 of |v_k|; the final fmaf / addition rounds once; the total, (d + 8) 2^-24, is
    doubled for margin.  A returned distance is within B of the model's for the returned label; the k-th order statistic moves by at
    most the largest perturbation of a candidate, so the model's k-th is within 2 max B of the returned k-th."""
    rng = np.random.default_rng(50 + d + metric)
    nlist, n, nq, k, nprobe = 8, 3000, 40, 10, 3
    cent = rng.standard_normal((nlist, d)).astype(F32) * 3
    x = (cent[rng.integers(0, nlist, n)] + rng.standard_normal((n, d))).astype(F32)
    xq = (cent[rng.integers(0, nlist, nq)] + rng.standard_normal((nq, d))).astype(F32)
    model = Model(metric, cent, x)
    D, I = _index(metric, cent, x).search(xq, k, nprobe=nprobe)
    Dm, _ = model.search(xq, k, nprobe)
    pairs, P = model.pairs(xq), sqr.probes(metric, cent, xq, nprobe)
    pos = np.empty(n, dtype=np.int64)
    for ids_l, _ in model.lists:
        pos[ids_l] = np.arange(ids_l.size)
    assert (I >= 0).all()
    for q in range(nq):
        l = model.of_row[I[q]]
        assert np.isin(l, P[q]).all()
        dis = np.array([pairs[a][0][q, b] for a, b in zip(l, pos[I[q]])], dtype=F64)
        B = np.array([pairs[a][1][q, b] for a, b in zip(l, pos[I[q]])])
        assert (np.abs(D[q].astype(F64) - dis) <= B).all(), q
        Bmax = max(pairs[a][1][q].max() for a in P[q])
        assert abs(float(D[q, k - 1]) - float(Dm[q, k - 1])) <= 2 * Bmax, q


@pytest.mark.parametrize("metric", [L2, IP])
def test_non_finite_rows_are_not_returned(metric, tmp_path):
    rng = np.random.default_rng(11 + metric)
    d, nlist, n = 12, 5, 40
    cent = _cent(nlist, d)
    of = rng.integers(0, nlist, n)
    x = (cent[of] + rng.integers(-3, 4, (n, d))).astype(F32)
    x[7, 2], x[7, 3] = 1e6, -1e6  # +inf and -inf in fp16; every query is positive there: inf - inf under inner product, a NaN
    xq = (cent[rng.integers(0, nlist, 9)] + rng.integers(-3, 4, (9, d))).astype(F32)
    xq[:, 2:4] += 5
    ix = _index(metric, cent, x)
    model = Model(metric, cent, x)
    assert np.isinf(model.h[7, 2:4]).all()
    D, I = ix.search(xq, 50, nprobe=nlist)
    _same((D, I), model.search(xq, 50, nlist), "a row of +-inf")
    assert not (I == 7).any() and (I[:, n - 1 :] == -1).all() and (D[:, n - 1 :] == (sqr.FLT_MAX if metric == L2 else -sqr.FLT_MAX)).all()
    # a NaN half, put into the image (the quantiser never sees it)
    path = str(tmp_path / "a.index")
    mf.write_index(ix, path)
    img = sqr.parse_ivfsq(path)
    l = next(l for l, (i, _) in enumerate(img["lists"]) if i.size and 7 not in i)
    img["lists"][l][1].view(np.float16)[0, 5] = np.nan
    gone = img["lists"][l][0][0]
    path2 = str(tmp_path / "b.index")
    sqr.write_ivfsq(path2, d, metric, cent, [], [], [(i, c.reshape(-1, d)) for i, c in img["lists"]], qtype=4, code_size=2 * d)
    D, I = mf.read_index(path2).search(xq, 50, nprobe=nlist)
    model.lists[l][1][0, 5] = np.nan
    _same((D, I), model.search(xq, 50, nlist), "a NaN row")
    assert not np.isin(I, [7, gone]).any() and (I[:, n - 2 :] == -1).all()


@pytest.mark.parametrize("metric", [L2, IP])
def test_a_query_alone_in_a_batch_and_again_gives_the_same_bits(metric):
    rng = np.random.default_rng(3 + metric)
    d, nlist = 40, 6
    cent = rng.standard_normal((nlist, d)).astype(F32) * 2
    x = (cent[rng.integers(0, nlist, 2500)] + rng.standard_normal((2500, d))).astype(F32)
    xq = (cent[rng.integers(0, 2, 70)] + rng.standard_normal((70, d))).astype(F32)
    ix = _index(metric, cent, x)
    D, I = ix.search(xq, 10, nprobe=3)
    _same(ix.search(xq, 10, nprobe=3), (D, I), "second run")
    for q in (0, 33, 69):
        D1, I1 = ix.search(xq[q : q + 1], 10, nprobe=3)
        _same((D1, I1), (D[q : q + 1], I[q : q + 1]), f"query {q} alone")


@pytest.mark.parametrize("metric", [L2, IP])
def test_the_rest_of_the_surface(metric, tmp_path):
    rng = np.random.default_rng(21 + metric)
    d, nlist, n, k, nprobe = 12, 5, 600, 8, 3
    cent = _cent(nlist, d)  # (integers again, of a wider range: every comparison below is exact and ties are rare)
    x = (cent[rng.integers(0, nlist, n)] + rng.integers(-60, 61, (n, d))).astype(F32)
    xq = (cent[rng.integers(0, nlist, 20)] + rng.integers(-60, 61, (20, d))).astype(F32)
    ids = rng.permutation(5 * n)[:n].astype(np.int64)
    ix = _index(metric, cent, x, ids)
    model = Model(metric, cent, x, ids)
    ref = model.search(xq, k, nprobe)
    _same(ix.search(xq, k, nprobe=nprobe), ref, "add_with_ids")
    assert ix.kind == mf.KIND_IVFSQ and ix.get_stat("sq_device_bytes") >= n * 2 * d
    for l, (ids_l, h_l) in enumerate(model.lists):  # the codes are FAISS's: little-endian fp16 of the residual
        got_ids, codes = ix.ivfsq_list(l)
        assert np.array_equal(got_ids, ids_l) and np.array_equal(codes.view(np.float16).view(np.uint16), h_l.view(np.uint16))
    # selectors
    keep = rng.random(n) < 0.5
    _same(ix.search(xq, k, nprobe=nprobe, sel=("bitmap", bitmap_from_ids(ids, keep))), model.search(xq, k, nprobe, keep_ids=ids[keep]), "bitmap")
    _same(ix.search(xq, k, nprobe=nprobe, sel=("batch", ids[keep])), model.search(xq, k, nprobe, keep_ids=ids[keep]), "batch")
    # reconstruct: f32(fp16(x - c)) + c, one f32 addition
    rec = (model.h.astype(F32) + cent[model.of_row]).astype(F32)
    assert np.array_equal(ix.reconstruct(int(ids[5])).view(np.uint32), rec[5].view(np.uint32))
    plain = _index(metric, cent, x)
    assert np.array_equal(plain.reconstruct_n(0, n).view(np.uint32), rec.view(np.uint32))
    # images and clones
    path = str(tmp_path / "fp16.index")
    mf.write_index(ix, path)
    img = sqr.parse_ivfsq(path)
    assert (img["qtype"], img["sq_code_size"], img["code_size"], img["by_residual"], img["vmin"]) == (4, 2 * d, 2 * d, 1, None)
    back = mf.read_index(path)
    assert back.sq_qtype == mf.QT_fp16 and back.is_trained and back.ntotal == n
    _same(back.search(xq, k, nprobe=nprobe), ref, "read_index")
    _same(ix.clone_to_gpu(ix.device).search(xq, k, nprobe=nprobe), ref, "clone")
    sqr.write_sq(str(tmp_path / "flat.index"), d, metric, [], [], np.zeros((0, d), np.uint8), qtype=4)  # the flat kind of the codec does not exist
    with pytest.raises(mf.FaissException, match="qtype = 4"):
        mf.read_index(str(tmp_path / "flat.index"))
    # merge_from of two halves equals one build
    a, b = _index(metric, cent, x[:300], ids[:300]), _index(metric, cent, x[300:], ids[300:])
    a.merge_from(b)
    assert a.ntotal == n and b.ntotal == 0
    _same(a.search(xq, k, nprobe=nprobe), ref, "merge_from")
    # remove_ids, then a search
    assert ix.remove_ids(("batch", ids[~keep])) == int((~keep).sum()) and ix.ntotal == int(keep.sum())
    (D, I), (Dr, Ir) = ix.search(xq, k, nprobe=nprobe), Model(metric, cent, x[keep], ids[keep]).search(xq, k, nprobe)
    # (IndexIVF::remove_ids fills a hole from the list's end, so positions differ from a fresh build's: equal distances may swap labels)
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32)) and np.array_equal(np.sort(I, axis=1), np.sort(Ir, axis=1)), "after remove_ids"


def test_the_door():
    rng = np.random.default_rng(5)
    d, nlist = 12, 5
    cent = _cent(nlist, d)
    x = (cent[rng.integers(0, nlist, 300)] + rng.standard_normal((300, d))).astype(F32)
    a, b = mf.GpuIndexIVFScalarQuantizer(d, nlist, mf.QT_8bit, L2), mf.index_factory(d, f"IVF{nlist},SQ8", L2)
    for ix in (a, b):
        ix.ivf_set_centroids(cent)
        ix.sq_set_trained(-4 * np.ones(d, F32), 8 * np.ones(d, F32))
        ix.add(x)
    _same(a.search(x[:20], 5, nprobe=2), b.search(x[:20], 5, nprobe=2), "QT_8bit against the factory's IVF<n>,SQ8")
    fp = _index(L2, cent, x)
    assert (fp.sq_qtype, a.sq_qtype, mf.index_factory(d, "Flat", L2).sq_qtype) == (4, 0, -1) == (mf.QT_fp16, mf.QT_8bit, -1)
    with pytest.raises(mf.FaissException, match="no trained range"):
        fp.sq_trained()
    for args in [(d, nlist, q) for q in (1, 2, 3, 5, 6, 7)] + [(d, nlist, 4, L2, False), (d, nlist, 4, 2), (2049, nlist, 4)]:
        with pytest.raises(mf.FaissException, match=NOT_IMPL):
            mf.GpuIndexIVFScalarQuantizer(*args)
    with pytest.raises(mf.FaissException, match="range search not implemented"):
        fp.range_search(x[:2], 1.0)
    with pytest.raises(mf.FaissException, match="This index type is not implemented"):
        fp.shard_to_gpus([0, 0])
