"""CPU-side checks of the IVF<n>,PQ<M> boundary: the header declares the kind and its two functions, the built library exports them,
the Python host lists them, the tests' own IwPQ writer / parser agree with each other, and the CPU model obeys its own rules on
cases small enough to check by hand."""
import ctypes
import os
import re

import numpy as np

import ivfpq_reference as ivr
import pq_reference as pqr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")
IVFPQ_FUNCTIONS = ["mvs_index_ivfpq_get_list", "mvs_index_ivfpq_list_size"]
L2, IP = ivr.L2, ivr.IP


def test_header_declares_the_ivfpq_kind_and_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+MVS_KIND_IVFPQ\s+6\b", src)
    assert re.search(r"\bint\s+mvs_index_ivfpq_get_list\s*\(", src)
    assert re.search(r"\bint64_t\s+mvs_index_ivfpq_list_size\s*\(", src)
    full = open(HEADER).read()
    assert "faiss_extension.cpp:675" in full  # the glue's IndexIVF cast is cited, the contract is written down
    for phrase in ("IwPQ", "probe rank", "by_residual is always true", "ivfpq_pair_block", "ivfpq_scan_rescans"):
        assert phrase in full, phrase


def test_library_exports_the_ivfpq_functions():
    import mi355_faiss as mf

    L = ctypes.CDLL(mf.LIB_PATH)
    missing = [n for n in IVFPQ_FUNCTIONS if not hasattr(L, n)]
    assert not missing, missing


def test_python_host_lists_the_ivfpq_functions():
    import mi355_faiss as mf

    assert mf.KIND_IVFPQ == 6
    for name in IVFPQ_FUNCTIONS:
        assert name in mf.DECLARED_SYMBOLS, name
    for method in ("ivfpq_list", "ivfpq_list_size"):
        assert callable(getattr(mf.Index, method)), method


def test_iwpq_image_round_trips_through_the_python_writer_and_parser():
    rng = np.random.default_rng(6)
    d, M, nlist = 12, 4, 5
    cb = pqr.synthetic_codebooks(rng, M, d // M)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    sizes = [7, 0, 1, 0, 30]
    lists, first = [], 0
    for n in sizes:
        lists.append((np.arange(first, first + n, dtype=np.int64), rng.integers(0, 256, size=(n, M), dtype=np.uint8)))
        first += n
    for id_map in (None, rng.permutation(1000)[:first].astype(np.int64)):
        for these in (lists, [lists[0]] + [(lists[1][0], lists[1][1])] * 4):  # 3 of 5 lists hold rows: "full"; 1 of 5: "sprs"
            img = ivr.parse_ivfpq(ivr.write_ivfpq(None, d, IP, cent, cb, these, nprobe=3, id_map=id_map))
            n = sum(i.size for i, _ in these)
            assert (img["d"], img["ntotal"], img["trained"], img["metric"], img["nlist"], img["nprobe"]) == (d, n, True, IP, nlist, 3)
            assert (img["by_residual"], img["code_size"], img["M"], img["nbits"]) == (1, M, M, 8)
            assert np.array_equal(img["centroids"].view(np.uint32), cent.view(np.uint32))
            assert np.array_equal(img["codebooks"].view(np.uint32), cb.view(np.uint32))
            for (ids_a, codes_a), (ids_b, codes_b) in zip(img["lists"], these):
                assert np.array_equal(ids_a, ids_b) and np.array_equal(codes_a, codes_b)
            assert (img["id_map"] is None) if id_map is None else np.array_equal(img["id_map"], id_map)
    # an index whose quantizer is still empty
    img = ivr.parse_ivfpq(ivr.write_ivfpq(None, d, L2, None, np.zeros_like(cb), [lists[1]] * nlist, trained=False))
    assert img["centroids"].shape == (0, d) and not img["trained"] and img["ntotal"] == 0


def _hand_case():
    cent = np.array([[1.0, 0.0], [4.0, 0.0]], dtype=np.float32)
    cb = np.zeros((1, 256, 2), dtype=np.float32)
    cb[0, :, 0] = 100.0 + np.arange(256)
    cb[0, 0] = (1.0, 0.0)
    cb[0, 1] = (-2.0, 0.0)  # list 0 with code 0 and list 1 with code 1 both reconstruct (2, 0)
    lists = [(np.array([10, 11], dtype=np.int64), np.zeros((2, 1), dtype=np.uint8)),
             (np.array([20, 21, 22], dtype=np.int64), np.ones((3, 1), dtype=np.uint8))]
    return cent, cb, lists


def test_model_orders_equal_sums_by_probe_rank_then_position():
    cent, cb, lists = _hand_case()
    # L2, query (0, 0): list 0 is rank 0, v = (-1, 0), T = |(-1, 0) - (1, 0)|^2 = 4; list 1: v = (-4, 0), T = |(-4, 0) - (-2, 0)|^2 = 4
    D, I = ivr.search(L2, cent, cb, lists, np.zeros((1, 2), dtype=np.float32), 7, 2)
    assert I[0].tolist() == [10, 11, 20, 21, 22, -1, -1]
    assert D[0, :5].tolist() == [4.0] * 5 and (D[0, 5:] == ivr.FLT_MAX).all()
    D, I = ivr.search(L2, cent, cb, lists, np.zeros((1, 2), dtype=np.float32), 3, 1)
    assert I[0].tolist() == [10, 11, -1] and D[0, :2].tolist() == [4.0, 4.0]
    # inner product, query (1, 0): list 1 is rank 0, base 4 + <(1, 0), (-2, 0)> = 2; list 0: base 1 + <(1, 0), (1, 0)> = 2
    q = np.array([[1.0, 0.0]], dtype=np.float32)
    D, I = ivr.search(IP, cent, cb, lists, q, 4, 9)
    assert I[0].tolist() == [20, 21, 22, 10] and D[0].tolist() == [2.0] * 4
    # a selector that empties the first probed list; labels through an id map
    id_map = np.arange(100, dtype=np.int64) * 3
    D, I = ivr.search(IP, cent, cb, lists, q, 3, 2, id_map=id_map, keep_ids=np.array([30, 33, 7], dtype=np.int64))
    assert I[0].tolist() == [30, 33, -1] and D[0, 2] == -ivr.FLT_MAX


def test_one_list_with_a_zero_centroid_is_the_pq_model():
    rng = np.random.default_rng(8)
    d, M = 12, 3
    cb = pqr.synthetic_codebooks(rng, M, d // M)
    xb = rng.standard_normal((700, d)).astype(np.float32)
    xb[rng.integers(0, 700, 90)] = xb[rng.integers(0, 700, 90)]
    xq = rng.standard_normal((6, d)).astype(np.float32)
    cent = np.zeros((1, d), dtype=np.float32)
    for metric in (L2, IP):
        lists = ivr.build_lists(metric, cent, cb, xb)
        assert np.array_equal(lists[0][0], np.arange(700)) and np.array_equal(lists[0][1], pqr.encode(cb, xb))
        for k in (1, 10, 800):
            D, I = ivr.search(metric, cent, cb, lists, xq, k, 1)
            Dr, Ir = pqr.search(cb, lists[0][1], xq, k, metric)
            assert np.array_equal(I, Ir) and np.array_equal(D.view(np.uint32), Dr.view(np.uint32)), (metric, k)
