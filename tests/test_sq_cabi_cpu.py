"""CPU-side checks of the SQ8 / IVF<n>,SQ8 boundary: the header declares the kinds, the functions and the contract's key phrases, the
built library exports the functions, the Python host lists them, the tests' own IxSQ / IwSq writers and parsers agree with each other,
and the CPU model obeys its own rules on cases small enough to check by hand."""
import ctypes
import os
import re

import numpy as np

import sq_reference as sqr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")
SQ_FUNCTIONS = ["mvs_index_sq_get_trained", "mvs_index_sq_set_trained", "mvs_index_sq_get_codes", "mvs_index_ivfsq_list_size",
                "mvs_index_ivfsq_get_list"]
L2, IP = sqr.L2, sqr.IP


def test_header_declares_the_sq_kinds_functions_and_contract():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+MVS_KIND_SQ\s+7\b", src)
    assert re.search(r"#define\s+MVS_KIND_IVFSQ\s+8\b", src)
    for name in SQ_FUNCTIONS:
        ret = "int64_t" if name.endswith("list_size") else "int"
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), src), name
    full = open(HEADER).read()
    for phrase in ("IxSQ", "IwSq", "no contraction", "vdiff[k] / 255.0f", "vmin[k] + 0.5f * s[k]", "(int)(255.0f * xi)", "a[k] + (float)c * s[k]",
                   "by_residual is always true", "probe rank", "sq_pair_block", "sq_rows_per_workgroup", "sq_scan_launches", "sq_scan_rescans",
                   "This index type is not implemented"):
        assert phrase in full, phrase


def test_library_exports_the_sq_functions():
    import mi355_faiss as mf

    L = ctypes.CDLL(mf.LIB_PATH)
    missing = [n for n in SQ_FUNCTIONS if not hasattr(L, n)]
    assert not missing, missing


def test_python_host_lists_the_sq_functions():
    import mi355_faiss as mf

    assert mf.KIND_SQ == 7 and mf.KIND_IVFSQ == 8
    for name in SQ_FUNCTIONS:
        assert name in mf.DECLARED_SYMBOLS, name
    for method in ("sq_trained", "sq_set_trained", "sq_codes", "ivfsq_list", "ivfsq_list_size"):
        assert callable(getattr(mf.Index, method)), method


def test_ixsq_image_round_trips_through_the_python_writer_and_parser():
    rng = np.random.default_rng(4)
    d, n = 5, 40
    vmin, vdiff = rng.standard_normal(d).astype(np.float32), rng.uniform(0.5, 2, d).astype(np.float32)
    codes = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    for ids in (None, rng.permutation(1000)[:n].astype(np.int64)):
        buf = sqr.write_sq(None, d, L2, vmin, vdiff, codes, ids=ids)
        assert buf[:4] == (b"IxSQ" if ids is None else b"IxMp")
        img = sqr.parse_sq(buf)
        assert (img["d"], img["ntotal"], img["trained"], img["metric"]) == (d, n, True, L2)
        assert (img["qtype"], img["rangestat"], img["rangestat_arg"], img["sq_code_size"]) == (0, 0, 0.0, d)
        assert np.array_equal(img["vmin"].view(np.uint32), vmin.view(np.uint32)) and np.array_equal(img["vdiff"].view(np.uint32), vdiff.view(np.uint32))
        assert np.array_equal(img["codes"], codes)
        assert (img["ids"] is None) if ids is None else np.array_equal(img["ids"], ids)
    # the block is 4 + 4 + 4 + 8 + 8 bytes, then the vector of 2 d floats
    head = 4 + struct_size_of_header()
    assert buf[:4] == b"IxMp" and sqr.write_sq(None, d, L2, vmin, vdiff, codes)[head : head + 12] == b"\0" * 12


def struct_size_of_header():
    return len(sqr._header(1, 0, True, 0))


def test_iwsq_image_round_trips_through_the_python_writer_and_parser():
    rng = np.random.default_rng(6)
    d, nlist = 12, 5
    vmin, vdiff = rng.standard_normal(d).astype(np.float32), rng.uniform(0.5, 2, d).astype(np.float32)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    sizes = [7, 0, 1, 0, 30]
    lists, first = [], 0
    for n in sizes:
        lists.append((np.arange(first, first + n, dtype=np.int64), rng.integers(0, 256, size=(n, d), dtype=np.uint8)))
        first += n
    for id_map in (None, rng.permutation(1000)[:first].astype(np.int64)):
        for these in (lists, [lists[0]] + [(lists[1][0], lists[1][1])] * 4):  # 3 of 5 lists hold rows: "full"; 1 of 5: "sprs"
            img = sqr.parse_ivfsq(sqr.write_ivfsq(None, d, IP, cent, vmin, vdiff, these, nprobe=3, id_map=id_map))
            n = sum(i.size for i, _ in these)
            assert (img["d"], img["ntotal"], img["trained"], img["metric"], img["nlist"], img["nprobe"]) == (d, n, True, IP, nlist, 3)
            assert (img["qtype"], img["sq_code_size"], img["code_size"], img["by_residual"]) == (0, d, d, 1)
            assert np.array_equal(img["centroids"].view(np.uint32), cent.view(np.uint32))
            assert np.array_equal(img["vmin"].view(np.uint32), vmin.view(np.uint32)) and np.array_equal(img["vdiff"].view(np.uint32), vdiff.view(np.uint32))
            for (ids_a, codes_a), (ids_b, codes_b) in zip(img["lists"], these):
                assert np.array_equal(ids_a, ids_b) and np.array_equal(codes_a, codes_b)
            assert (img["id_map"] is None) if id_map is None else np.array_equal(img["id_map"], id_map)
    # an index whose quantizer is still empty
    img = sqr.parse_ivfsq(sqr.write_ivfsq(None, d, L2, None, np.zeros(d), np.zeros(d), [lists[1]] * nlist, trained=False))
    assert img["centroids"].shape == (0, d) and not img["trained"] and img["ntotal"] == 0


def test_a_constant_dimension_gives_code_0_and_decodes_to_vmin():
    x = np.array([[1.0, 7.5, -3.0], [2.0, 7.5, 5.0], [4.0, 7.5, 0.0]], dtype=np.float32)
    vmin, vdiff = sqr.train_range(x)
    assert vmin.tolist() == [1.0, 7.5, -3.0] and vdiff.tolist() == [3.0, 0.0, 8.0]
    codes = sqr.encode(vmin, vdiff, x)
    assert codes[:, 1].tolist() == [0, 0, 0]
    assert codes[:, 0].tolist() == [0, 85, 255] and codes[:, 2].tolist() == [0, 255, 95]  # (int)(255 * 1/3), (int)(255 * 3/8 = 95.6)
    dec = sqr.decode(vmin, vdiff, codes)
    assert dec[:, 1].tolist() == [7.5, 7.5, 7.5]  # s = 0, a = vmin
    # a row outside the range: a constant dimension still gives 0
    assert sqr.encode(vmin, vdiff, np.array([[0.0, 100.0, 0.0]], dtype=np.float32))[0, 1] == 0


def test_values_outside_the_range_clamp_to_0_and_255():
    vmin, vdiff = np.array([-1.0, 10.0], dtype=np.float32), np.array([2.0, 5.0], dtype=np.float32)
    y = np.array([[-1.5, 9.0], [-1.0, 10.0], [1.0, 15.0], [1.0001, 400.0], [-1e30, 1e30]], dtype=np.float32)
    assert sqr.encode(vmin, vdiff, y).tolist() == [[0, 0], [0, 0], [255, 255], [255, 255], [0, 255]]


def test_in_range_values_decode_within_half_a_step():
    rng = np.random.default_rng(9)
    d, n = 7, 5000
    x = (rng.standard_normal((n, d)) * rng.uniform(0.01, 100, d) + rng.uniform(-50, 50, d)).astype(np.float32)
    vmin, vdiff = sqr.train_range(x)
    a, s = sqr.derived(vmin, vdiff)
    assert np.array_equal(s, (vdiff / np.float32(255)).astype(np.float32))
    dec = sqr.decode(vmin, vdiff, sqr.encode(vmin, vdiff, x))
    bound = 0.5 * s.astype(np.float64) + 2 * np.spacing(np.abs(x)).astype(np.float64)
    err = np.abs(dec.astype(np.float64) - x.astype(np.float64))
    assert (err <= bound).all(), (err - bound).max()


def test_models_chains_and_orders_on_a_hand_case():
    # s = 1, a = 0: codes decode to themselves
    vmin, vdiff = np.full(2, -0.5, dtype=np.float32), np.full(2, 255.0, dtype=np.float32)
    codes = np.array([[3, 4], [0, 5], [5, 0], [3, 4]], dtype=np.uint8)
    assert sqr.decode(vmin, vdiff, codes).tolist() == [[3, 4], [0, 5], [5, 0], [3, 4]]
    q = np.zeros((1, 2), dtype=np.float32)
    D, I = sqr.sq_search(L2, vmin, vdiff, codes, q, 6)
    assert I[0].tolist() == [0, 1, 2, 3, -1, -1] and D[0, :4].tolist() == [25.0] * 4 and (D[0, 4:] == sqr.FLT_MAX).all()
    D, I = sqr.sq_search(IP, vmin, vdiff, codes, np.array([[1.0, 1.0]], dtype=np.float32), 3, labels=np.array([40, 30, 20, 10]), keep=[1, 1, 0, 1])
    assert I[0].tolist() == [40, 10, 30] and D[0].tolist() == [7.0, 7.0, 5.0]
    # IVF: list 0 (centroid (1, 0)) code (1, 0) and list 1 (centroid (4, 0)) code ... reconstruct x = c + dec
    cent = np.array([[1.0, 0.0], [4.0, 0.0]], dtype=np.float32)
    lists = [(np.array([10, 11], dtype=np.int64), np.array([[1, 0], [1, 0]], dtype=np.uint8)),
             (np.array([20, 21, 22], dtype=np.int64), np.array([[2, 0]] * 3, dtype=np.uint8))]
    # L2, query (0, 0): list 0 at rank 0, v = (-1, 0), t = (-2, 0): 4; list 1, v = (-4, 0), t = (-6, 0): 36
    D, I = sqr.ivf_search(L2, cent, vmin, vdiff, lists, q, 4, 2)
    assert I[0].tolist() == [10, 11, 20, 21] and D[0].tolist() == [4.0, 4.0, 36.0, 36.0]
    # inner product, query (1, 0): list 1 at rank 0, base 4 + 2 = 6; list 0: base 1 + 1 = 2
    D, I = sqr.ivf_search(IP, cent, vmin, vdiff, lists, np.array([[1.0, 0.0]], dtype=np.float32), 4, 9)
    assert I[0].tolist() == [20, 21, 22, 10] and D[0].tolist() == [6.0, 6.0, 6.0, 2.0]
    # one list with a zero centroid is the SQ8 model
    rng = np.random.default_rng(3)
    xb = rng.standard_normal((300, 6)).astype(np.float32)
    xq = rng.standard_normal((5, 6)).astype(np.float32)
    vmin, vdiff = sqr.train_range(xb)
    zero = np.zeros((1, 6), dtype=np.float32)
    for metric in (L2, IP):
        lists = sqr.build_lists(metric, zero, vmin, vdiff, xb)
        assert np.array_equal(lists[0][1], sqr.encode(vmin, vdiff, xb))
        D, I = sqr.ivf_search(metric, zero, vmin, vdiff, lists, xq, 20, 1)
        Dr, Ir = sqr.sq_search(metric, vmin, vdiff, lists[0][1], xq, 20)
        assert np.array_equal(I, Ir) and np.array_equal(D.view(np.uint32), Dr.view(np.uint32))
