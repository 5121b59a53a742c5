"""CPU-side checks of the PQ<M> boundary: the header declares the kind and its four functions, the built library exports them,
the Python host lists them, and the tests' own IxPq writer / parser agree with each other."""
import ctypes
import os
import re

import numpy as np

import pq_reference as pqr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")
PQ_FUNCTIONS = ["mvs_index_pq_info", "mvs_index_pq_get_centroids", "mvs_index_pq_set_centroids", "mvs_index_pq_get_codes"]


def _header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_pq_kind_and_functions():
    src = _header_code()
    assert re.search(r"#define\s+MVS_KIND_PQ\s+5\b", src)
    for name in PQ_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
    # the convention of the file: the glue's cast is cited, the contract is written down
    full = open(HEADER).read()
    assert "faiss_extension.cpp:704" in full
    assert "multiple of the number of subquantizers" in full


def test_library_exports_the_pq_functions():
    import mi355_faiss as mf

    L = ctypes.CDLL(mf.LIB_PATH)
    missing = [n for n in PQ_FUNCTIONS if not hasattr(L, n)]
    assert not missing, missing


def test_python_host_lists_the_pq_functions():
    import mi355_faiss as mf

    for name in PQ_FUNCTIONS:
        assert name in mf.DECLARED_SYMBOLS, name
    for method in ("pq_info", "pq_centroids", "pq_set_centroids", "pq_codes"):
        assert callable(getattr(mf.Index, method)), method


def test_ixpq_image_round_trips_through_the_python_writer_and_parser():
    rng = np.random.default_rng(5)
    cb = pqr.synthetic_codebooks(rng, 4, 3)
    codes = rng.integers(0, 256, size=(37, 4), dtype=np.uint8)
    for ids in (None, rng.permutation(1000)[:37].astype(np.int64)):
        img = pqr.parse_pq(pqr.write_pq(None, 12, 1, cb, codes, ids=ids))
        assert (img["d"], img["ntotal"], img["M"], img["nbits"], img["metric"], img["trained"]) == (12, 37, 4, 8, 1, True)
        assert (img["search_type"], img["encode_signs"], img["polysemous_ht"]) == (0, 0, 33)
        assert np.array_equal(img["centroids"].view(np.uint32), cb.view(np.uint32))
        assert np.array_equal(img["codes"], codes)
        assert (img["ids"] is None) if ids is None else np.array_equal(img["ids"], ids)


def test_reference_model_orders_ties_by_row_and_pads():
    # 3 sub-vectors of one dimension, rows that repeat: the model's own rules on a case small enough to check by hand
    cb = np.zeros((1, 256, 1), dtype=np.float32)
    cb[0, :, 0] = np.arange(256)
    x = np.array([[3.0], [1.0], [3.0], [2.4], [1.0]], dtype=np.float32)
    codes = pqr.encode(cb, x)
    assert codes[:, 0].tolist() == [3, 1, 3, 2, 1]
    D, I = pqr.search(cb, codes, np.array([[1.0]], dtype=np.float32), 7, 1)
    assert I[0].tolist() == [1, 4, 3, 0, 2, -1, -1]
    assert D[0, :5].tolist() == [0.0, 0.0, 1.0, 4.0, 4.0] and (D[0, 5:] == pqr.FLT_MAX).all()
    D, I = pqr.search(cb, codes, np.array([[1.0]], dtype=np.float32), 2, 0, keep=[True, False, True, True, True])
    assert I[0].tolist() == [0, 2] and D[0].tolist() == [3.0, 3.0]
