"""CPU-side checks of the reconstruct boundary: the header declares the six functions and the contract's key phrases, the built library
exports them, the Python host lists them, and the CPU model (tests/reconstruct_reference.py) agrees with itself on a hand-computed case per
kind."""
import ctypes
import os
import re

import numpy as np
import pytest

import faiss_format as ff
import hnswsq_reference as hsr
import ivfpq_reference as ivr
import pq_reference as pqr
import reconstruct_reference as rcr
import refine_reference as rfr
import sq_reference as sqr
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
SIGNATURES = {
    "mvs_index_reconstruct": r"mvs_index\s*\*\s*ix\s*,\s*int64_t\s+key\s*,\s*float\s*\*\s*recons",
    "mvs_index_reconstruct_n": r"mvs_index\s*\*\s*ix\s*,\s*int64_t\s+i0\s*,\s*int64_t\s+ni\s*,\s*float\s*\*\s*recons",
    "mvs_index_reconstruct_batch": r"mvs_index\s*\*\s*ix\s*,\s*int64_t\s+n\s*,\s*const\s+int64_t\s*\*\s*keys\s*,\s*float\s*\*\s*recons",
    "mvs_index_search_and_reconstruct": r"mvs_index\s*\*\s*ix\s*,\s*int64_t\s+n\s*,\s*const\s+float\s*\*\s*x\s*,\s*int64_t\s+k\s*,\s*float\s*\*\s*distances\s*,"
                                        r"\s*int64_t\s*\*\s*labels\s*,\s*float\s*\*\s*recons\s*,\s*const\s+mvs_search_params\s*\*\s*params",
    "mvs_index_reconstruct_batch_device": r"mvs_index\s*\*\s*ix\s*,\s*int64_t\s+n\s*,\s*const\s+int64_t\s*\*\s*d_keys\s*,\s*float\s*\*\s*d_recons\s*,"
                                          r"\s*void\s*\*\s*stream",
    "mvs_index_search_and_reconstruct_device": r"mvs_index\s*\*\s*ix\s*,\s*int64_t\s+n\s*,\s*const\s+float\s*\*\s*d_x\s*,\s*int64_t\s+k\s*,"
                                               r"\s*float\s*\*\s*d_distances\s*,\s*int64_t\s*\*\s*d_labels\s*,\s*float\s*\*\s*d_recons\s*,"
                                               r"\s*const\s+mvs_search_params\s*\*\s*params\s*,\s*void\s*\*\s*stream",
}


def test_header_declares_the_reconstruct_functions_and_contract():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in SIGNATURES.items():
        assert re.search(r"int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), src), name
    full = open(HEADER).read()
    for phrase in ("key not found", "reconstruct not implemented for this type of index", "last", "left untouched", "0xFF", "DEPARTURE",
                   "'ni == 0 || (i0 >= 0 && i0 + ni <= ntotal)' failed", "recon_pq_lds"):
        assert phrase in full, phrase
    section = full[full.index("---- reconstruct:") :]
    assert section.count("DEPARTURE") >= 2  # no make_direct_map; IDMap serves as IDMap2


def test_library_exports_the_reconstruct_functions():
    import mi355_faiss as mf

    L = ctypes.CDLL(mf.LIB_PATH)
    missing = [n for n in SIGNATURES if not hasattr(L, n)]
    assert not missing, missing


def test_python_host_lists_the_reconstruct_functions():
    import mi355_faiss as mf

    for name in SIGNATURES:
        assert name in mf.DECLARED_SYMBOLS, name
    for m in ("reconstruct", "reconstruct_n", "reconstruct_batch", "search_and_reconstruct", "reconstruct_batch_torch", "search_and_reconstruct_torch"):
        assert callable(getattr(mf.Index, m)), m


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_flat_idmap_and_last_added_wins():
    x = np.arange(12, dtype=np.float32).reshape(4, 3)
    m = rcr.load(ff.dumps({"kind": "flat", "d": 3, "metric": L2, "x": x}))
    assert m.ntotal == 4 and m.reconstruct(2).tolist() == [6.0, 7.0, 8.0]
    assert np.array_equal(m.reconstruct_n(1, 2), x[1:3]) and np.array_equal(m.reconstruct_batch([3, 0, 3]), x[[3, 0, 3]])
    assert m.reconstruct_n(0, 0).shape == (0, 3) and m.reconstruct_n(9, 0).shape == (0, 3)  # ni == 0 passes the range check
    for bad in (4, -1):
        with pytest.raises(rcr.OutOfRange):
            m.reconstruct(bad)
    with pytest.raises(rcr.OutOfRange):
        m.reconstruct_n(2, 3)
    # IDMap: external ids, 7 twice -- the row added last wins; a range of keys must exist whole
    ids = np.array([7, 5, 7, 6], dtype=np.int64)
    m = rcr.load(ff.dumps({"kind": "idmap", "d": 3, "metric": L2, "ids": ids, "sub": {"kind": "flat", "d": 3, "metric": L2, "x": x}}))
    assert m.reconstruct(7).tolist() == x[2].tolist() and m.reconstruct(5).tolist() == x[1].tolist()
    assert np.array_equal(m.reconstruct_n(5, 3), x[[1, 3, 2]])
    with pytest.raises(rcr.KeyNotFound) as e:
        m.reconstruct_batch([5, 99, 6, 98])
    assert e.value.args[0] == 99  # the FIRST missing key in batch order
    with pytest.raises(rcr.KeyNotFound):
        m.reconstruct_n(4, 3)
    # labels of a search: -1 gives a row of 0xFF bytes
    R = m.of_labels(np.array([[6, -1], [7, 5]]))
    assert R.shape == (2, 2, 3) and (R[0, 1].view(np.uint8) == 0xFF).all() and np.array_equal(R[1], x[[2, 1]]) and np.array_equal(R[0, 0], x[3])


def test_pq_and_sq_decode_on_hand_cases():
    cb = np.zeros((2, 256, 2), dtype=np.float32)
    cb[0, :, 0], cb[0, :, 1] = np.arange(256), -np.arange(256)
    cb[1, :, 0], cb[1, :, 1] = 1000 + np.arange(256), 0.5
    codes = np.array([[3, 0], [255, 7]], dtype=np.uint8)
    assert rcr.pq_decode(cb, codes).tolist() == [[3.0, -3.0, 1000.0, 0.5], [255.0, -255.0, 1007.0, 0.5]]
    m = rcr.load(pqr.write_pq(None, 4, L2, cb, codes, ids=np.array([40, 40], dtype=np.int64)))
    assert m.reconstruct(40).tolist() == [255.0, -255.0, 1007.0, 0.5]
    # s = 1, a = 0: codes decode to themselves
    vmin, vdiff = np.full(2, -0.5, dtype=np.float32), np.full(2, 255.0, dtype=np.float32)
    sc = np.array([[3, 4], [0, 5], [5, 0]], dtype=np.uint8)
    m = rcr.load(sqr.write_sq(None, 2, IP, vmin, vdiff, sc))
    assert m.reconstruct_n(0, 3).tolist() == [[3, 4], [0, 5], [5, 0]]
    # a range where the two roundings show: a + (float)c s, each operation on its own
    rng = np.random.default_rng(1)
    xb = rng.standard_normal((50, 5)).astype(np.float32)
    vmin, vdiff = sqr.train_range(xb)
    codes = sqr.encode(vmin, vdiff, xb)
    a, s = sqr.derived(vmin, vdiff)
    want = (a + (codes.astype(np.float32) * s).astype(np.float32)).astype(np.float32)
    m = rcr.load(sqr.write_sq(None, 5, L2, vmin, vdiff, codes))
    assert np.array_equal(_bits(m.reconstruct_n(0, 50)), _bits(want))


def test_ivf_kinds_on_the_two_list_hand_cases():
    # IVF,SQ8 (tests/test_sq_cabi_cpu.py): list 0, centroid (1, 0), code (1, 0); list 1, centroid (4, 0), code (2, 0); x = c + dec
    vmin, vdiff = np.full(2, -0.5, dtype=np.float32), np.full(2, 255.0, dtype=np.float32)
    cent = np.array([[1.0, 0.0], [4.0, 0.0]], dtype=np.float32)
    lists = [(np.array([10, 11], dtype=np.int64), np.array([[1, 0], [1, 0]], dtype=np.uint8)),
             (np.array([20, 21, 22], dtype=np.int64), np.array([[2, 0]] * 3, dtype=np.uint8))]
    m = rcr.load(sqr.write_ivfsq(None, 2, L2, cent, vmin, vdiff, lists))
    assert m.bare_ivf and m.reconstruct(10).tolist() == [2.0, 0.0] and m.reconstruct(22).tolist() == [6.0, 0.0]
    # a bare IVF kind: reconstruct_n writes the ids present at id - i0 and leaves the others untouched
    out = np.full((4, 2), -7.0, dtype=np.float32)
    m.reconstruct_n(9, 4, out=out)
    assert out.tolist() == [[-7.0, -7.0], [2.0, 0.0], [2.0, 0.0], [-7.0, -7.0]]
    with pytest.raises(rcr.KeyNotFound):
        m.reconstruct(12)
    # IVF,PQ (tests/test_ivfpq_cabi_cpu.py): list 0 with code 0 and list 1 with code 1 both reconstruct (2, 0)
    cb = np.zeros((1, 256, 2), dtype=np.float32)
    cb[0, :, 0] = 100.0 + np.arange(256)
    cb[0, 0] = (1.0, 0.0)
    cb[0, 1] = (-2.0, 0.0)
    plists = [(np.array([10, 11], dtype=np.int64), np.zeros((2, 1), dtype=np.uint8)), (np.array([20, 21, 22], dtype=np.int64), np.ones((3, 1), dtype=np.uint8))]
    m = rcr.load(ivr.write_ivfpq(None, 2, L2, cent, cb, plists))
    assert [m.reconstruct(k).tolist() for k in (10, 11, 20, 21, 22)] == [[2.0, 0.0]] * 5
    # under IDMap the stored ids are row numbers of the map: external 300 is stored id 2 (list 1)
    plists2 = [(np.array([0, 3], dtype=np.int64), np.array([[5], [0]], dtype=np.uint8)), (np.array([1, 2], dtype=np.int64), np.array([[1], [6]], dtype=np.uint8))]
    m = rcr.load(ivr.write_ivfpq(None, 2, L2, cent, cb, plists2, id_map=np.array([100, 200, 300, 100], dtype=np.int64)))
    assert m.reconstruct(300).tolist() == [110.0, 0.0] and m.reconstruct(200).tolist() == [2.0, 0.0]
    assert m.reconstruct(100).tolist() == [2.0, 0.0]  # rows 0 and 3 carry 100: row 3 (code 0 in list 0) was added last
    # the residual first, then ONE addition of the centroid: (a + c s) + centroid, not a + (c s + centroid)
    rng = np.random.default_rng(2)
    c2 = rng.standard_normal((2, 3)).astype(np.float32)
    xb = rng.standard_normal((40, 3)).astype(np.float32)
    of_row, _ = sqr.assign(L2, c2, xb)
    vmin, vdiff = sqr.train_range(sqr.residuals(c2, xb, of_row))
    lists = sqr.build_lists(L2, c2, vmin, vdiff, xb)
    m = rcr.load(sqr.write_ivfsq(None, 3, L2, c2, vmin, vdiff, lists))
    for l, (ids_l, codes_l) in enumerate(lists):
        want = (sqr.decode(vmin, vdiff, codes_l) + c2[l]).astype(np.float32)
        assert np.array_equal(_bits(m.reconstruct_batch(ids_l)), _bits(want))
    # duplicates in different lists: the image alone cannot say which came last, the arrival lists can
    dup = [(np.array([5], dtype=np.int64), np.array([[1, 0]], dtype=np.uint8)), (np.array([5], dtype=np.int64), np.array([[2, 0]], dtype=np.uint8))]
    vmin, vdiff = np.full(2, -0.5, dtype=np.float32), np.full(2, 255.0, dtype=np.float32)
    img = sqr.write_ivfsq(None, 2, L2, cent, vmin, vdiff, dup)
    assert rcr.load(img, of_row=[1, 0]).reconstruct(5).tolist() == [2.0, 0.0]  # the row of list 0 arrived second
    assert rcr.load(img, of_row=[0, 1]).reconstruct(5).tolist() == [6.0, 0.0]


def test_ivfflat_hnsw_and_refine_images():
    x = np.arange(10, dtype=np.float32).reshape(5, 2)
    quant = {"kind": "flat", "d": 2, "metric": L2, "x": np.zeros((2, 2), dtype=np.float32)}
    iv = {"kind": "ivfflat", "d": 2, "metric": L2, "is_trained": True, "nlist": 2, "nprobe": 1, "quantizer": quant,
          "lists": [(np.array([9, 7], dtype=np.int64), x[[0, 1]]), (np.array([5, 7, 3], dtype=np.int64), x[[2, 3, 4]])]}
    m = rcr.load(ff.dumps(iv))
    assert m.bare_ivf and m.reconstruct(9).tolist() == x[0].tolist() and m.reconstruct(3).tolist() == x[4].tolist()
    out = np.full((8, 2), np.float32(-1.5))
    m.reconstruct_n(2, 8, out=out)  # ids 3, 5, 7, 9 at rows 1, 3, 5, 7
    assert (out[0::2] == -1.5).all() and np.array_equal(out[[1, 3, 7]], x[[4, 2, 0]])
    assert np.array_equal(out[5], x[3])  # without arrival lists the later image entry of id 7 wins ...
    m.set_arrival([1, 0, 1, 0, 1])  # ... rows arrived as: list 1, list 0, list 1, list 0, list 1 -> id 7 of list 0 is arrival 3, of list 1 arrival 2
    assert m.reconstruct(7).tolist() == x[1].tolist()
    # the refine store's rows under an id map
    vmin, vdiff = np.full(2, -0.5, dtype=np.float32), np.full(2, 255.0, dtype=np.float32)
    base = sqr.write_sq(None, 2, L2, vmin, vdiff, np.zeros((5, 2), dtype=np.uint8))
    m = rcr.load(rfr.write_refine(None, 2, L2, base, x, 2.0, id_map=np.array([50, 40, 30, 20, 10], dtype=np.int64)))
    assert m.reconstruct(30).tolist() == x[2].tolist() and np.array_equal(m.reconstruct_batch([10, 50]), x[[4, 0]])
    # HNSW,SQ8: the storage's decoded codes
    g = hsr.full_graph(2, dict(levels=np.ones(3, dtype=np.int32), offsets=np.array([0, 4, 8, 12], dtype=np.uint64),
                               neighbors=np.full(12, -1, dtype=np.int32), entry_point=0, max_level=0))
    codes = np.array([[3, 4], [0, 5], [5, 0]], dtype=np.uint8)
    m = rcr.load(hsr.write_hnswsq(None, 2, L2, g, vmin, vdiff, codes))
    assert m.reconstruct_n(0, 3).tolist() == [[3, 4], [0, 5], [5, 0]]
