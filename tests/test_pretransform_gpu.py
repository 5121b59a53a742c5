"""Pre-transform indexes ("PCA<o>,...", "PCAW<o>,...", "L2norm,...") on the device against the CPU model of tests/pretransform_reference.py.
The apply path, L2norm, the wrapper against its sub-index, files and refusals are compared bit for bit (labels array_equal, floats as uint32);
PCA training is judged against numpy.linalg.eigh in f64 with the bounds the header's rules give, never against the code under test."""
import os
import subprocess

import numpy as np
import pytest

import ivfpq_reference as ivr
import pq_reference as pqr
import pretransform_reference as ptr
import range_reference as rgr
import refine_reference as rfr
import sq_reference as sqr
from helpers import bitmap_from_ids
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "duckdb-faiss-ext_amd", "host", "boundary_driver")
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
NOT_YET = "This index type is not implemented on the MI355X path yet"


def _mf():
    import mi355_faiss as mf

    return mf


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_floats(y, ym, what):
    """bit for bit, a NaN matching any NaN"""
    y, ym = np.asarray(y, dtype=np.float32), np.asarray(ym, dtype=np.float32)
    assert y.shape == ym.shape, what
    nan = np.isnan(ym)
    assert np.array_equal(np.isnan(y), nan), f"{what}: NaN positions differ"
    bad = (_bits(y) != _bits(ym)) & ~nan
    assert not bad.any(), f"{what}: {bad.sum()} values differ, first at {np.argwhere(bad)[0].tolist()}"


def _same(D, I, Dr, Ir, what):
    assert np.array_equal(I, Ir), f"{what}: labels differ in {(I != Ir).sum()} slots, first query {np.argwhere(I != Ir)[0][0]}"
    assert np.array_equal(_bits(D), _bits(Dr)), f"{what}: distances differ in {(_bits(D) != _bits(Dr)).sum()} slots"


def _outcome(fn):
    """what a call gives, or the text it fails with: two indexes that must behave alike are compared on either"""
    try:
        return ("ok", fn())
    except _mf().FaissException as e:
        return ("error", e.msg[e.msg.index(" at ") :].split(": ", 1)[1])  # "Error in <function> at <file>: <text>"


def _same_outcome(a, b, what):
    assert a[0] == b[0], f"{what}: {a[0]} against {b[0]}: {a[1] if a[0] == 'error' else b[1]}"
    if a[0] == "error":
        assert a[1] == b[1], what
        return False
    return True


def _hostile_rows(rng, n, d):
    """normal rows; from 31 rows on also +-0, subnormals, 1e30-sized values and a row holding a NaN"""
    x = rng.standard_normal((n, d)).astype(np.float32)
    if n >= 31:
        x[0] = np.where(np.arange(d) % 2 == 0, np.float32(0.0), np.float32(-0.0))
        x[1] = (rng.standard_normal(d) * 1e-40).astype(np.float32)
        x[2] = (rng.standard_normal(d) * 1e30).astype(np.float32)
        x[3, d // 2] = np.nan
        x[4, : (d + 1) // 2] = 0.0
        x[5] = (x[5] * 1e-22).astype(np.float32)  # (products fall among the subnormals)
    return x


def _linear_index(tmp_path, d_in, d_out):
    """an empty index whose chain is one linear slot d_in -> d_out over Flat: from the factory where it makes one (d_out <= d_in), otherwise
    from a crafted "LTra" image"""
    mf = _mf()
    if d_out <= d_in:
        return mf.index_factory(d_in, f"PCA{d_out},Flat", L2)
    path = str(tmp_path / f"lt_{d_in}_{d_out}.index")
    ptr.write_pretransform(path, d_in, L2, [dict(fourcc=b"LTra", d_in=d_in, d_out=d_out, A=np.zeros((d_out, d_in)), b=None)],
                           rfr.flat_image(d_out, L2, np.zeros((0, d_out), dtype=np.float32)))
    return mf.read_index(path)


# ------------------------------------------------------------------------------------------ 1. apply, bit for bit
@pytest.mark.parametrize("d_in", [1, 2, 3, 31, 33, 64, 130])
def test_apply_is_the_k_ordered_chain_plus_one_addition(d_in, tmp_path):
    mf = _mf()
    rng = np.random.default_rng(100 + d_in)
    x = _hostile_rows(rng, 257, d_in)
    for d_out in (1, 5, 32, 33, 100):
        ix = _linear_index(tmp_path, d_in, d_out)
        assert ix.kind == mf.KIND_PRETRANSFORM and ix.pretransform_count == 1
        A = rng.standard_normal((d_out, d_in)).astype(np.float32)
        A[0, 0] = -0.0
        b = rng.standard_normal(d_out).astype(np.float32)
        for bias in (None, b):
            ix.pretransform_set_linear(0, A, bias)
            t = ix.pretransform_info(0)
            assert t == dict(type=mf.VT_LINEAR, d_in=d_in, d_out=d_out, have_bias=bias is not None, is_trained=True)
            ym = ptr.linear(A, bias, x)  # (rows are independent: the model of the 257 rows serves every smaller batch)
            for n in (1, 31, 32, 33, 257):
                xs = x[257 - n :] if n < 31 else x[:n]
                y = ix.pretransform_apply(xs)
                _same_floats(y, ym[257 - n :] if n < 31 else ym[:n], f"d_in = {d_in}, d_out = {d_out}, n = {n}, bias = {bias is not None}")
                assert ix.get_stat("pretransform_apply_launches") == 1
        if d_out == 33:  # the device-resident entry, at an address that is not 16-byte aligned
            import torch

            buf = torch.zeros(257 * d_in + 1, dtype=torch.float32, device="cuda")
            buf[1:] = torch.from_numpy(x.reshape(-1)).cuda()
            y = ix.pretransform_apply_torch(buf[1:].view(257, d_in)).cpu().numpy()
            _same_floats(y, ym, f"d_in = {d_in}, d_out = 33, device rows")


def test_add_in_two_workspace_chunks_equals_adds_per_row_block():
    """L2norm,PCA64,SQ8 at d = 64: a chunk's workspace is 64 staged floats, an id slot and two buffers of 64 floats = 776 bytes a row, so
    256 MB hold 345 920 rows and 350 000 rows need two chunks"""
    mf = _mf()
    rng = np.random.default_rng(5)
    d, n = 64, 350000
    x = rng.random((n, d), dtype=np.float32) - np.float32(0.5)
    A = (rng.standard_normal((d, d)) / 8).astype(np.float32)
    b = rng.standard_normal(d).astype(np.float32)
    vmin, vdiff = np.full(d, -2.0, dtype=np.float32), np.full(d, 4.0, dtype=np.float32)
    codes = []
    for blocks in ([n], [100000, 100000, 100000, 50000]):
        ix = mf.index_factory(d, "L2norm,PCA64,SQ8", L2)
        ix.pretransform_set_linear(1, A, b)
        ix.pretransform_sub.sq_set_trained(vmin, vdiff)
        assert ix.is_trained
        r0 = 0
        for nb in blocks:
            ix.add(x[r0 : r0 + nb])
            r0 += nb
        assert ix.ntotal == n
        if len(blocks) == 1:
            assert ix.get_stat("pretransform_apply_launches") == 4  # two chunks of two transforms
            assert 0 < ix.get_stat("pretransform_workspace_bytes") <= 256 << 20
        codes.append(ix.pretransform_sub.sq_codes())
    assert np.array_equal(codes[0], codes[1])
    for rows in (slice(0, 257), slice(345800, 346057), slice(n - 257, n)):  # (the second spans the chunk boundary)
        y = ptr.apply_chain([dict(type=ptr.VT_NORM), dict(type=ptr.VT_LINEAR, A=A, b=b)], x[rows])
        assert np.array_equal(codes[0][rows], sqr.encode(vmin, vdiff, y))


# ------------------------------------------------------------------------------------------ 2. L2norm, bit for bit
@pytest.mark.parametrize("d", [1, 3, 64, 130])
def test_l2norm_is_fvec_renorm_l2(d):
    mf = _mf()
    rng = np.random.default_rng(200 + d)
    x = rng.standard_normal((70, d)).astype(np.float32)
    x[7] = 0.0
    x[9, d // 2] = np.nan
    x[11] = (x[11] * 1e-30).astype(np.float32)  # (the squares underflow towards the subnormals)
    x[12] = (x[12] * 1e25).astype(np.float32)   # (the sum overflows: inv = 0)
    ix = mf.index_factory(d, "L2norm,Flat", IP)
    assert ix.is_trained and ix.pretransform_info(0) == dict(type=mf.VT_NORM, d_in=d, d_out=d, have_bias=False, is_trained=True)
    with np.errstate(all="ignore"):
        ym = ptr.l2norm(x)
    y = ix.pretransform_apply(x)
    _same_floats(y, ym, f"L2norm d = {d}")
    assert np.array_equal(_bits(y[7]), _bits(x[7])) and np.isnan(y[9, d // 2])


def test_chain_of_three_equals_the_models_composition():
    mf = _mf()
    rng = np.random.default_rng(21)
    x = _hostile_rows(rng, 100, 9)
    A, b = rng.standard_normal((4, 9)).astype(np.float32), rng.standard_normal(4).astype(np.float32)
    ix = mf.index_factory(9, "L2norm,PCA4,L2norm,Flat", L2)
    assert ix.pretransform_count == 3 and not ix.is_trained
    ix.pretransform_set_linear(1, A, b)
    assert ix.is_trained
    with np.errstate(all="ignore"):
        ym = ptr.apply_chain([dict(type=ptr.VT_NORM), dict(type=ptr.VT_LINEAR, A=A, b=b), dict(type=ptr.VT_NORM)], x)
    _same_floats(ix.pretransform_apply(x), ym, "L2norm,PCA4,L2norm")
    assert ix.get_stat("pretransform_apply_launches") == 3


# ------------------------------------------------------------------------------------------ 3. wrapper == sub-index of the transformed rows
_DATA = {}


def _data():
    if not _DATA:
        rng = np.random.default_rng(33)
        scale = np.linspace(2.0, 0.3, 24)
        _DATA["x"] = (rng.standard_normal((600, 24)) * scale[None, :] + 0.5).astype(np.float32)
        _DATA["xq"] = (rng.standard_normal((40, 24)) * scale[None, :] + 0.5).astype(np.float32)
        _DATA["ids"] = (np.arange(600, dtype=np.int64) * 3 + 7)
    return _DATA["x"], _DATA["xq"], _DATA["ids"]


@pytest.mark.parametrize("idmap", [False, True])
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("sub", ["Flat", "IVF4,Flat", "PQ4", "IVF4,PQ2", "SQ8", "IVF4,SQ8", "HNSW8"])
def test_wrapper_equals_the_sub_index_of_the_transformed_rows(sub, metric, idmap):
    mf = _mf()
    x, xq, ids = _data()
    pre = "IDMap," if idmap else ""
    made = _outcome(lambda: mf.index_factory(8, pre + sub, metric))
    wrapped = _outcome(lambda: mf.index_factory(24, pre + "PCA8," + sub, metric))
    if made[0] == "error":  # a metric the sub-index does not take: the wrapper refuses in the sub-index's words
        assert wrapped[0] == "error" and wrapped[1].replace("PCA8,", "") == made[1]
        return
    ref, ix = made[1], wrapped[1]
    assert (ix.kind == mf.KIND_IDMAP and ix.index.kind == mf.KIND_PRETRANSFORM) if idmap else ix.kind == mf.KIND_PRETRANSFORM
    assert ix.d == 24 and ix.pretransform_sub.d == 8 and ix.pretransform_sub.kind == (ref.index if idmap else ref).kind
    assert not ix.is_trained
    if sub.startswith("HNSW"):
        ix.set_option("hnsw_build_waves", 1)
        ref.set_option("hnsw_build_waves", 1)
    ix.train(x)
    assert ix.is_trained and ix.pretransform_info(0)["is_trained"]
    A, b = ix.pretransform_get_linear(0)
    y, yq = ptr.linear(A, b, x), ptr.linear(A, b, xq)
    _same_floats(ix.pretransform_apply(x), y, "the transformed rows")
    s = ix.pretransform_sub
    if sub.startswith("IVF"):
        ref.ivf_set_centroids(s.ivf_centroids())
    if "PQ" in sub:
        ref.pq_set_centroids(s.pq_centroids())
    if "SQ" in sub:
        ref.sq_set_trained(*s.sq_trained())
    assert ref.is_trained
    for rows in (slice(0, 350), slice(350, 600)):  # (the same add batches on both sides: an HNSW build depends on them, as FAISS's does)
        if idmap:
            ix.add_with_ids(x[rows], ids[rows])
            ref.add_with_ids(y[rows], ids[rows])
        else:
            ix.add(x[rows])
            ref.add(y[rows])
    if not idmap:
        a, c = _outcome(lambda: ix.add_with_ids(x[:2], ids[:2])), _outcome(lambda: ref.add_with_ids(y[:2], ids[:2]))
        if a[0] == "error" or c[0] == "error":  # a bare sub-index that refuses ids refuses with its own text
            _same_outcome(a, c, "add_with_ids")
            labels = np.arange(600, dtype=np.int64)
        else:
            labels = np.concatenate([np.arange(600, dtype=np.int64), ids[:2]])
    if idmap:
        labels = ids
    assert ix.ntotal == ref.ntotal == len(labels)
    nprobes = (1, 4) if sub.startswith("IVF") else (0,)

    def compare(stage, keep_mask):
        lab = labels[keep_mask]
        some = lab[:: 3]
        sels = [None, ("bitmap", bitmap_from_ids(labels, np.isin(labels, some))), ("batch", some)]
        for k in (1, 10):
            for sel in sels:
                for nprobe in nprobes:
                    what = f"{pre}PCA8,{sub} metric {metric} {stage} k = {k} sel = {sel and sel[0]} nprobe = {nprobe}"
                    got = _outcome(lambda: ix.search(xq, k, nprobe=nprobe, sel=sel))
                    want = _outcome(lambda: ref.search(yq, k, nprobe=nprobe, sel=sel))
                    if _same_outcome(got, want, what):
                        _same(*got[1], *want[1], what)
                        if sel is not None:
                            assert np.isin(got[1][1], np.concatenate([some, [-1]])).all(), what
        assert ix.last_kernel_info() == ref.last_kernel_info()

    compare("as built", np.ones(len(labels), dtype=bool))
    if sub in ("Flat", "IVF4,Flat"):
        D10, _ = ref.search(yq, 10, nprobe=4)
        radius = float(np.median(D10[:, -1]))
        for nprobe in nprobes:
            got, want = ix.range_search(xq, radius, nprobe=nprobe), ref.range_search(yq, radius, nprobe=nprobe)
            assert want[0][-1] > 0 and rgr.same(got, want), f"range_search nprobe = {nprobe}"
    gone = labels[::2]
    a, c = _outcome(lambda: ix.remove_ids(("batch", gone))), _outcome(lambda: ref.remove_ids(("batch", gone)))
    if _same_outcome(a, c, "remove_ids"):
        assert a[1] == c[1] > 0
        assert ix.ntotal == ref.ntotal
        keep = ~np.isin(labels, gone)
        if not idmap and not sub.startswith("IVF"):  # (rows close up: a bare Flat, PQ or SQ8 index renumbers its labels)
            labels = np.arange(ix.ntotal, dtype=np.int64)
            keep = np.ones(len(labels), dtype=bool)
        compare("after remove_ids", keep)
        if sub in ("Flat", "IVF4,Flat"):
            got, want = ix.range_search(xq, radius, nprobe=nprobes[-1]), ref.range_search(yq, radius, nprobe=nprobes[-1])
            assert rgr.same(got, want), "range_search after remove_ids"
    for call in (lambda: ix.reconstruct(int(labels[0])), lambda: ix.reconstruct_n(0, 1), lambda: ix.reconstruct_batch(labels[:2]),
                 lambda: ix.search_and_reconstruct(xq, 2)):
        with pytest.raises(mf.FaissException, match="not implemented"):
            call()


def test_cosine_is_l2norm_flat_under_inner_product():
    mf = _mf()
    x, xq, ids = _data()
    with np.errstate(all="ignore"):
        y, yq = ptr.l2norm(x), ptr.l2norm(xq)
    assert np.abs(np.linalg.norm(y.astype(np.float64), axis=1) - 1).max() < 1e-6
    for pre in ("", "IDMap,"):
        ix, ref = mf.index_factory(24, pre + "L2norm,Flat", IP), mf.index_factory(24, pre + "Flat", IP)
        assert ix.is_trained
        if pre:
            ix.add_with_ids(x, ids)
            ref.add_with_ids(y, ids)
        else:
            ix.add(x)
            ref.add(y)
        for k in (1, 10):
            _same(*ix.search(xq, k), *ref.search(yq, k), f"{pre}L2norm,Flat k = {k}")
            assert ix.last_kernel_info() == ref.last_kernel_info()
        # the statistics entry points look through the chain: the searching kernels are the sub-index's
        assert ix.collect_stats() == ref.collect_stats() and ix.prefilter_stats() == ref.prefilter_stats() and ix.ivf_probe_stats() == ref.ivf_probe_stats()
        D, _ = ix.search(xq, 1)
        assert (D <= 1.0 + 1e-6).all() and (D > 0).all()


# ------------------------------------------------------------------------------------------ 4. PCA training
def test_pca_training_against_eigh():
    mf = _mf()
    x = ptr.planted()  # d_in = 12, n = 4096, variances 2^-i along a random orthonormal basis, plus an offset; seed 7
    m = ptr.pca_train(x, 5)
    rel, ab = ptr.spectrum_gaps(m["lam64"])
    assert rel >= 0.25 and ab >= 1e-4, (rel, ab)
    images = []
    for trial in range(2):
        ix = mf.index_factory(12, "PCA5,Flat", L2)
        assert not ix.is_trained and not ix.pretransform_info(0)["is_trained"]
        ix.train(x)
        assert ix.is_trained
        assert ix.pretransform_info(0) == dict(type=mf.VT_PCA, d_in=12, d_out=5, have_bias=True, is_trained=True)
        A, b = ix.pretransform_get_linear(0)
        mean, ev = ix.pretransform_get_pca(0)
        images.append(b"".join(a.tobytes() for a in (A, b, mean, ev)))
    assert images[0] == images[1], "training twice on the same rows gives other bits"
    A64, V = A.astype(np.float64), m["V64"]
    dots = np.abs(np.einsum("ik,ik->i", A64, V[:5]))
    print("PCA5: 1 - |<a_i, v_i>| =", (1 - dots).tolist(), " max |A A^T - I| =", np.abs(A64 @ A64.T - np.eye(5)).max(),
          " eigenvalue error =", np.abs(ev / m["lam64"] - 1).max())
    assert (dots >= 1 - 2.0 ** -23).all(), dots
    assert np.abs(A64 @ A64.T - np.eye(5)).max() <= 2.0 ** -22
    assert all(a[int(np.argmax(np.abs(a)))] > 0 for a in A), "the sign rule"
    assert (np.diff(ev) <= 0).all() and np.abs(ev / m["lam64"] - 1).max() <= 1e-6
    assert np.abs(mean - m["mean"]).max() <= 1e-6
    assert np.array_equal(_bits(b), _bits(ptr.pca_bias(A, mean))), "b is not the model's b of the device's own A and mean"
    # a transform that is trained is left alone: other rows change nothing
    ix.train((x[:100] * 3).astype(np.float32))
    assert np.array_equal(_bits(ix.pretransform_get_linear(0)[0]), _bits(A))


def test_pcaw_whitens_the_training_rows():
    mf = _mf()
    x = ptr.planted()
    ix = mf.index_factory(12, "PCAW5,IVF4,Flat", L2)
    ix.train(x)
    assert ix.is_trained and ix.pretransform_sub.is_trained
    y = ix.pretransform_apply(x).astype(np.float64)
    var = y.var(axis=0)
    print("PCAW5: variances", var.tolist(), " means", y.mean(axis=0).tolist())
    assert np.abs(var - 1.0).max() <= 1e-4 and np.abs(y.mean(axis=0)).max() <= 1e-4
    A, b = ix.pretransform_get_linear(0)
    assert np.array_equal(_bits(b), _bits(ptr.pca_bias(A, ix.pretransform_get_pca(0)[0])))


def test_pca_training_needs_rows():
    mf = _mf()
    x = ptr.planted()
    ix = mf.index_factory(12, "PCA5,Flat", L2)
    with pytest.raises(mf.FaissException, match=r"n = 4 .*d_out = 5"):
        ix.train(x[:4])
    with pytest.raises(mf.FaissException, match=r"n = 0"):
        ix.train(x[:0])
    assert not ix.is_trained
    with pytest.raises(mf.FaissException, match="'is_trained'"):
        ix.add(x[:3])
    with pytest.raises(mf.FaissException, match="'is_trained'"):
        ix.search(x[:3], 1)
    with pytest.raises(mf.FaissException, match="'is_trained'"):
        ix.pretransform_apply(x[:3])
    with pytest.raises(mf.FaissException, match="not trained"):
        ix.pretransform_get_linear(0)
    ix.train(x[:5])  # n = d_out: enough
    assert ix.is_trained


# ------------------------------------------------------------------------------------------ 5. files
def test_write_read_round_trip(tmp_path):
    mf = _mf()
    x, xq, ids = _data()
    for desc, metric in (("PCA8,IVF4,Flat", L2), ("IDMap,PCAW8,L2norm,SQ8", IP)):
        ix = mf.index_factory(24, desc, metric)
        ix.train(x)
        if desc.startswith("IDMap"):
            ix.add_with_ids(x, ids)
        else:
            ix.add(x)
        path = str(tmp_path / "a.index")
        mf.write_index(ix, path)
        back = mf.read_index(path)
        assert (back.kind, back.d, back.ntotal, back.is_trained, back.metric_type) == (ix.kind, 24, 600, True, metric)
        assert back.pretransform_count == ix.pretransform_count
        for i in range(ix.pretransform_count):
            assert back.pretransform_info(i) == ix.pretransform_info(i)
        for a, c in zip(ix.pretransform_get_linear(0) + ix.pretransform_get_pca(0), back.pretransform_get_linear(0) + back.pretransform_get_pca(0)):
            assert np.array_equal(_bits(a), _bits(c))
        for k in (1, 10):
            _same(*back.search(xq, k, nprobe=2), *ix.search(xq, k, nprobe=2), f"{desc} after write -> read")
        raw = open(path, "rb").read()
        img = ptr.parse_pretransform(raw)
        assert (img["d"], img["ntotal"], img["trained"], img["metric"]) == (24, 600, True, metric)
        t = img["chain"][0]
        A, b = ix.pretransform_get_linear(0)
        mean, ev = ix.pretransform_get_pca(0)
        assert t["fourcc"] == b"PcAm" and t["have_bias"] and t["is_trained"] and (t["d_in"], t["d_out"]) == (24, 8)
        assert t["eigen_power"] == (-0.5 if "PCAW" in desc else 0.0) and t["epsilon"] == 0.0 and not t["random_rotation"] and t["balanced_bins"] == 0
        assert np.array_equal(_bits(t["A"]), _bits(A)) and np.array_equal(_bits(t["b"]), _bits(b))
        assert np.array_equal(_bits(t["mean"]), _bits(mean)) and np.array_equal(_bits(t["eigenvalues"]), _bits(ev)) and t["PCAMat"].size == 24 * 24
        if "L2norm" in desc:
            assert img["chain"][1]["fourcc"] == b"VNrm" and img["chain"][1]["norm"] == 2.0 and np.array_equal(img["id_map"], ids)
            assert img["sub"][:4] == b"IxSQ"
        else:
            assert img["sub"][:4] == b"IwFl" and img["id_map"] is None
        mf.write_index(back, str(tmp_path / "b.index"))
        assert open(str(tmp_path / "b.index"), "rb").read() == raw
    # a set matrix is written as "LTra", without a bias if none was set
    ix = mf.index_factory(6, "PCA2,Flat", L2)
    ix.pretransform_set_linear(0, np.arange(12, dtype=np.float32).reshape(2, 6))
    mf.write_index(ix, str(tmp_path / "c.index"))
    t = ptr.parse_pretransform(open(str(tmp_path / "c.index"), "rb").read())["chain"][0]
    assert t["fourcc"] == b"LTra" and not t["have_bias"] and t["b"].size == 0 and t["A"].reshape(-1).tolist() == list(range(12))


def _crafted_chain(rng, fourcc, d_in, d_out):
    if fourcc == b"VNrm":
        return [dict(fourcc=b"VNrm", d_in=d_in, d_out=d_in, norm=2.0), dict(fourcc=b"LTra", d_in=d_in, d_out=d_out, A=rng.standard_normal((d_out, d_in)), b=None)]
    A = rng.standard_normal((d_out, d_in)).astype(np.float32)
    t = dict(fourcc=fourcc, d_in=d_in, d_out=d_out, A=A, b=None if fourcc in (b"LTra", b"rrot") else rng.standard_normal(d_out).astype(np.float32))
    if fourcc in (b"PCAm", b"PcAm"):
        t.update(eigen_power=0.0, epsilon=0.0, mean=rng.standard_normal(d_in), eigenvalues=np.arange(d_in, 0, -1), PCAMat=rng.standard_normal((d_in, d_in)))
    return [t]


def _model_chain(chain):
    return [dict(type=ptr.VT_NORM) if t["fourcc"] == b"VNrm" else dict(type=ptr.VT_LINEAR, A=t["A"], b=t["b"]) for t in chain]


@pytest.mark.parametrize("fourcc", [b"LTra", b"rrot", b"PCAm", b"PcAm", b"VNrm"])
def test_crafted_images_load_and_search_as_the_model_says(fourcc, tmp_path):
    """what FAISS writes for a rotation in front of an index (an OPQ matrix is a plain "LTra"), over a Flat and an IVF4,PQ2 sub-image"""
    mf = _mf()
    rng = np.random.default_rng(50)
    d_in, d_out, n = 10, 8, 300  # (d_out > d_in for "LTra": no factory string makes one)
    if fourcc == b"LTra":
        d_in, d_out = 6, 8
    chain = _crafted_chain(rng, fourcc, d_in, d_out)
    xq = rng.standard_normal((30, d_in)).astype(np.float32)
    yq = ptr.apply_chain(_model_chain(chain), xq)
    rows = rng.standard_normal((n, d_out)).astype(np.float32)
    path = str(tmp_path / "x.index")
    # over Flat
    ptr.write_pretransform(path, d_in, L2, chain, rfr.flat_image(d_out, L2, rows), ntotal=n)
    ix = mf.read_index(path)
    assert ix.kind == mf.KIND_PRETRANSFORM and (ix.d, ix.ntotal, ix.is_trained) == (d_in, n, True) and ix.pretransform_sub.kind == mf.KIND_FLAT
    want_type = {b"LTra": mf.VT_LINEAR, b"rrot": mf.VT_LINEAR, b"PCAm": mf.VT_PCA, b"PcAm": mf.VT_PCA, b"VNrm": mf.VT_NORM}[fourcc]
    assert ix.pretransform_info(0)["type"] == want_type
    _same_floats(ix.pretransform_apply(xq), yq, f"{fourcc} apply")
    ref = mf.index_factory(d_out, "Flat", L2)
    ref.add(rows)
    for k in (1, 10):
        _same(*ix.search(xq, k), *ref.search(yq, k), f"{fourcc} over Flat k = {k}")
    # the image written back: PCA's vectors survive, "rrot" becomes "LTra"
    mf.write_index(ix, str(tmp_path / "y.index"))
    img = ptr.parse_pretransform(open(str(tmp_path / "y.index"), "rb").read())
    assert [t["fourcc"] for t in img["chain"]] == [{b"rrot": b"LTra", b"PCAm": b"PcAm"}.get(t["fourcc"], t["fourcc"]) for t in chain]
    if fourcc in (b"PCAm", b"PcAm"):
        assert np.array_equal(img["chain"][0]["mean"], np.float32(chain[0]["mean"])) and img["chain"][0]["PCAMat"].size == d_in * d_in
    # over IVF4,PQ2, under IDMap
    cent = rows[:4].copy()
    cb = pqr.synthetic_codebooks(rng, 2, d_out // 2)
    lists = ivr.build_lists(L2, cent, cb, rows)
    id_map = np.arange(n, dtype=np.int64) * 2 + 11
    ptr.write_pretransform(path, d_in, L2, chain, ivr.write_ivfpq(None, d_out, L2, cent, cb, lists, nprobe=2), ntotal=n, id_map=id_map)
    ix = mf.read_index(path)
    assert ix.kind == mf.KIND_IDMAP and ix.index.kind == mf.KIND_PRETRANSFORM and ix.pretransform_sub.kind == mf.KIND_IVFPQ and ix.ntotal == n
    for k, nprobe in ((1, 1), (10, 4)):
        Dm, Im = ivr.search(L2, cent, cb, lists, yq, k, nprobe, id_map=id_map)
        _same(*ix.search(xq, k, nprobe=nprobe), Dm, Im, f"{fourcc} over IDMap,IVF4,PQ2 k = {k}")


def test_images_that_do_not_hold_together_are_refused(tmp_path):
    mf = _mf()
    path = str(tmp_path / "bad.index")
    flat8 = rfr.flat_image(8, L2, np.zeros((0, 8), dtype=np.float32))
    A = np.zeros((8, 10), dtype=np.float32)

    def refused(chain, pattern, sub=flat8, d=10, cut=None):
        buf = ptr.write_pretransform(None, d, L2, chain, sub)
        with open(path, "wb") as f:
            f.write(buf if cut is None else buf[:cut])
        with pytest.raises(mf.FaissException, match=pattern):
            mf.read_index(path)

    ok = dict(fourcc=b"LTra", d_in=10, d_out=8, A=A, b=None)
    assert mf.read_index(ptr.write_pretransform(path, 10, L2, [ok], flat8) and path).kind == mf.KIND_PRETRANSFORM
    refused([dict(ok, A=np.zeros(79))], r"A holds 79 values, not d_in \* d_out = 10 \* 8")
    refused([dict(ok, b=np.zeros(7), have_bias=True)], r"b holds 7 values, not d_out = 8")
    refused([dict(ok, b=None, have_bias=True)], r"b holds 0 values, not d_out = 8")
    refused([dict(fourcc=b"VNrm", d_in=9, d_out=9, norm=2.0), ok], r"do not join: transform 0 takes d_in = 9 where 10 arrive")
    refused([dict(fourcc=b"VNrm", d_in=10, d_out=10, norm=2.0), dict(ok, d_in=12, A=np.zeros((8, 12)))], r"do not join: transform 1 takes d_in = 12 where 10 arrive")
    refused([dict(ok, d_out=7, A=np.zeros((7, 10)))], r"output dimension 7 is not the sub-index's d = 8")
    refused([dict(fourcc=b"VNrm", d_in=10, d_out=10, norm=1.0), ok], r"norm = 1 is not implemented")
    for cc in (b"RmDT", b"VCnt", b"Viqt", b"Viqm", b"opqm"):
        refused([dict(fourcc=cc, d_in=10, d_out=8)], cc.decode())
    whole = len(ptr.write_pretransform(None, 10, L2, [ok], flat8))
    for cut in (whole - 1, whole - len(flat8) + 2, 60, 37):
        refused([ok], "unexpected end of file", cut=cut)
    refused([ok] * 5, r"chain of 5 transforms")


# ------------------------------------------------------------------------------------------ 6. factory and refusals
def test_factory_strings_and_refusals():
    mf = _mf()
    parse = "could not parse index string"
    for desc in ("PCAR4,Flat", "PCAWR4,Flat", "RR4,Flat", "ITQ4,Flat", "Pad16,Flat", "LDA4,Flat", "L2norm,PCAR4,Flat", "IDMap,RR4,Flat"):
        with pytest.raises(mf.FaissException, match=NOT_YET + ": " + desc + "$"):
            mf.index_factory(8, desc, L2)
    for desc in ("OPQ4,PQ4", "OPQ4_8,IVF4,PQ4", "PCA4,PQ4,RFlat", "L2norm,SQ8,Refine(Flat)"):
        with pytest.raises(mf.FaissException, match=NOT_YET):
            mf.index_factory(8, desc, L2)
    with pytest.raises(mf.FaissException, match=r"PCA9: the output dimension 9 must lie in \[1, d_in = 8\]"):
        mf.index_factory(8, "PCA9,Flat", L2)
    with pytest.raises(mf.FaissException, match=r"PCA5: the output dimension 5 must lie in \[1, d_in = 4\]"):
        mf.index_factory(8, "PCA4,PCA5,Flat", L2)
    with pytest.raises(mf.FaissException, match=r"output dimension 0"):
        mf.index_factory(8, "PCA0,Flat", L2)
    for desc in ("PCA4", "L2norm", "PCA4,L2norm", "PCA4,", "PCA4,IDMap,Flat", "PCAx4,Flat", "PCA4,Nonsense"):
        with pytest.raises(mf.FaissException, match=parse):
            mf.index_factory(8, desc, L2)
    with pytest.raises(mf.FaissException, match=NOT_YET + ".*at most 4"):
        mf.index_factory(8, "L2norm,L2norm,L2norm,L2norm,L2norm,Flat", L2)
    with pytest.raises(mf.FaissException, match=NOT_YET + ".*d_in = 2049"):
        mf.index_factory(2049, "PCA4,Flat", L2)
    # a good index: kind, count, info, sub
    ix = mf.index_factory(8, "IDMap2,L2norm,PCA4,PCAW2,L2norm,IVF4,SQ8", IP)
    assert ix.kind == mf.KIND_IDMAP and ix.index.kind == mf.KIND_PRETRANSFORM and ix.d == 8 and ix.metric_type == IP
    assert ix.pretransform_count == 4 and ix.index.pretransform_count == 4
    assert [ix.pretransform_info(i)["type"] for i in range(4)] == [mf.VT_NORM, mf.VT_PCA, mf.VT_PCA, mf.VT_NORM]
    assert [(ix.pretransform_info(i)["d_in"], ix.pretransform_info(i)["d_out"]) for i in range(4)] == [(8, 8), (8, 4), (4, 2), (2, 2)]
    s = ix.pretransform_sub
    assert s.kind == mf.KIND_IVFSQ and s.d == 2 and s.nlist == 4
    assert mf.index_factory(8, "Flat", L2).pretransform_sub is None and mf.index_factory(8, "Flat", L2).pretransform_count == -1
    with pytest.raises(mf.FaissException, match="transform 4 of a chain of 4"):
        ix.pretransform_info(4)
    with pytest.raises(mf.FaissException, match="not a PreTransform index"):
        mf.index_factory(8, "Flat", L2).pretransform_info(0)
    with pytest.raises(mf.FaissException, match="normalisation"):
        ix.pretransform_set_linear(0, np.zeros((8, 8)))
    # set_linear: only while the index is empty; add before train
    ix = mf.index_factory(8, "PCA4,Flat", L2)
    x = np.random.default_rng(1).standard_normal((20, 8)).astype(np.float32)
    with pytest.raises(mf.FaissException, match="'is_trained'"):
        ix.add(x)
    ix.pretransform_set_linear(0, np.eye(4, 8), np.ones(4))
    assert ix.is_trained and ix.pretransform_info(0)["type"] == mf.VT_LINEAR
    with pytest.raises(mf.FaissException, match="not a trained PCA"):
        ix.pretransform_get_pca(0)
    ix.add(x)
    with pytest.raises(mf.FaissException, match="only while ntotal == 0"):
        ix.pretransform_set_linear(0, np.eye(4, 8))
    D, I = ix.search(x[:3], 1)
    assert I[:, 0].tolist() == [0, 1, 2] and (D == 0).all()
    with pytest.raises(mf.FaissException, match="add_with_ids not implemented"):
        ix.add_with_ids(x[:2], np.arange(2))
    # sharding and the reconstruct family
    with pytest.raises(mf.FaissException, match="This index type is not implemented$"):
        ix.clone_to_gpu(-1)
    with pytest.raises(mf.FaissException, match="This index type is not implemented$"):
        ix.shard_to_gpus([0])
    for call in (lambda: ix.reconstruct(0), lambda: ix.reconstruct_n(0, 2), lambda: ix.reconstruct_batch([0, 1]), lambda: ix.search_and_reconstruct(x[:2], 1)):
        with pytest.raises(mf.FaissException, match="reconstruct not implemented for this type of index"):
            call()
    # placement: a clone on the same device answers alike; to_gpu in place keeps answering
    c = ix.clone_to_gpu(0)
    _same(*c.search(x, 3), *ix.search(x, 3), "clone_to_gpu(0)")
    ix.to_gpu(0)
    _same(*c.search(x, 3), *ix.search(x, 3), "to_gpu(0)")


def test_sharding_by_environment_is_refused():
    env = dict(os.environ, MVS_DEVICES="0,0")
    code = ("import mi355_faiss as mf\n"
            "try:\n    mf.index_factory(8, 'PCA4,Flat', 1)\n    print('made')\nexcept mf.FaissException as e:\n    print(e.msg)\n")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"), env.get("PYTHONPATH", "")])
    out = subprocess.run([os.sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120).stdout
    assert out.strip().endswith("This index type is not implemented"), out


# ------------------------------------------------------------------------------------------ 7. the boundary driver
def test_boundary_driver_pretransform_mode_prints_what_pyhost_returns():
    """factory -> train -> add -> search through the faiss:: classes of compat/faiss: the same labels and distance bits as the Python host
    gives for the same inputs (the driver's rows are the same generator's: see its usage text)"""
    mf = _mf()
    if not os.path.exists(DRIVER):
        pytest.fail("host/boundary_driver is not built")
    d, n, nq, k = 24, 500, 8, 5
    r = subprocess.run([DRIVER, "pretransform", str(d), str(n), str(nq), str(k)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("pretransform ")]
    assert lines, r.stdout
    seen = {}
    for ln in lines:
        f = ln.split()
        seen.setdefault(f[1], []).append((int(f[2]), [int(v) for v in f[3 : 3 + k]], [int(v, 16) for v in f[3 + k : 3 + 2 * k]]))
    i = np.arange(n * d, dtype=np.int64)
    x = (((i * 2654435761 + 12345) % 1000003).astype(np.float64) / 1000003.0 - 0.5).astype(np.float32).reshape(n, d)
    c = np.arange(d, dtype=np.float64)
    x = (x * (2.0 + (0.25 - 2.0) * c / (d - 1)).astype(np.float32)[None, :]).astype(np.float32)
    for desc, metric in (("PCA8,Flat", L2), ("L2norm,Flat", IP), ("IDMap,PCAW8,IVF4,Flat", L2)):
        ix = mf.index_factory(d, desc, metric)
        ix.train(x)
        if desc.startswith("IDMap"):
            ix.add_with_ids(x, np.arange(n, dtype=np.int64) * 7 + 3)
        else:
            ix.add(x)
        D, I = ix.search(x[:nq], k, nprobe=2)
        got = seen[desc]
        assert len(got) == nq, desc
        for q, labels, dbits in got:
            assert labels == I[q].tolist() and dbits == _bits(D[q]).tolist(), f"{desc} query {q}"
