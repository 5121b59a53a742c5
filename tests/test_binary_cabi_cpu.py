"""CPU-side checks of the binary indexes (include/mi355_faiss.h "binary indexes"): the header declares the family and carries the
contract's key phrases, the library exports it, the Python host lists it, the entry point fails loudly without a GPU, and the CPU model of
tests/binary_reference.py agrees with cases worked out by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

import binary_reference as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")

FUNCTIONS = [
    "mvs_binary_index_factory", "mvs_binary_index_free", "mvs_binary_index_d", "mvs_binary_index_code_size", "mvs_binary_index_ntotal",
    "mvs_binary_index_kind", "mvs_binary_index_idmap_sub", "mvs_binary_index_add", "mvs_binary_index_add_with_ids",
    "mvs_binary_index_search", "mvs_binary_index_range_search", "mvs_binary_index_reset", "mvs_binary_index_reconstruct",
    "mvs_binary_index_reconstruct_n", "mvs_binary_index_add_device", "mvs_binary_index_search_device", "mvs_binary_index_set_option",
    "mvs_binary_index_get_stat", "mvs_write_index_binary", "mvs_read_index_binary",
]  # fmt: skip


def test_header_declares_the_family_and_states_the_contract():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mvs_[a-z0-9_]+)\s*\(", code))
    assert not [f for f in FUNCTIONS if f not in declared]
    assert "typedef struct mvs_binary_index mvs_binary_index;" in code
    for phrase in ("IBxF", "IBMp", "2147483647", "'d % 8 == 0' failed", "ham < radius"):
        assert phrase in src, phrase
    section = src[src.index("---- binary indexes") :]
    assert section.count("DEPARTURE") >= 2


def test_library_exports_and_python_host_lists_the_family():
    import mi355_faiss as mf

    L = ctypes.CDLL(mf.LIB_PATH)
    assert not [f for f in FUNCTIONS if not hasattr(L, f)]
    assert not [f for f in FUNCTIONS if f not in mf.DECLARED_SYMBOLS]
    for m in ("add", "add_with_ids", "search", "range_search", "reset", "reconstruct", "reconstruct_n", "add_torch", "search_torch",
              "set_option", "get_stat", "train"):  # fmt: skip
        assert callable(getattr(mf.IndexBinary, m)), m
    for p in ("d", "code_size", "ntotal", "kind", "index", "is_trained", "metric_type"):
        assert isinstance(getattr(mf.IndexBinary, p), property), p
    assert callable(mf.index_binary_factory) and callable(mf.read_index_binary) and callable(mf.write_index_binary)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a box without a GPU")
def test_fails_loudly_without_gpu():
    import mi355_faiss as mf

    with pytest.raises(mf.FaissException, match="no CPU fallback"):
        mf.index_binary_factory(64, "BFlat")


def test_model_hand_computed_search():
    xb = np.array([[0x00], [0xFF], [0x0F], [0x0F]], dtype=np.uint8)
    xq = np.array([[0x0F]], dtype=np.uint8)
    assert br.ham(xq, xb).tolist() == [[4, 4, 0, 0]]
    D, I = br.search(xb, xq, 4)
    assert list(zip(D[0].tolist(), I[0].tolist())) == [(0, 2), (0, 3), (4, 0), (4, 1)]
    D, I = br.search(xb, xq, 6)  # k > n pads
    assert D[0].tolist() == [0, 0, 4, 4, 2147483647, 2147483647] and I[0].tolist() == [2, 3, 0, 1, -1, -1]
    assert D.dtype == np.int32 and I.dtype == np.int64
    D, I = br.search(xb, xq, 2, id_map=[70, 5, -3, 9])  # labels through the id map, ties still by row
    assert I[0].tolist() == [-3, 9]


def test_model_selectors():
    xb = np.array([[0x00], [0xFF], [0x0F], [0x0F]], dtype=np.uint8)
    xq = np.array([[0x0F]], dtype=np.uint8)
    D, I = br.search(xb, xq, 2, sel=("batch", [1, 1, 77]))  # admits row 1 alone; a duplicate and a stranger are harmless
    assert D[0].tolist() == [4, 2147483647] and I[0].tolist() == [1, -1]
    D, I = br.search(xb, xq, 2, sel=("bitmap", np.array([0b0100], np.uint8)))  # bit 2
    assert D[0].tolist() == [0, 2147483647] and I[0].tolist() == [2, -1]
    # the bitmap tests the external id under IDMap: a negative id and one beyond the bitmap are no members
    D, I = br.search(xb, xq, 4, sel=("bitmap", np.array([0xFF], np.uint8)), id_map=[-1, 8, 3, 1 << 40])
    assert D[0].tolist() == [0] + [2147483647] * 3 and I[0].tolist() == [3, -1, -1, -1]
    assert br.member(("bitmap", np.zeros(0, np.uint8)), [0, 1]).tolist() == [False, False]


def test_model_range_search():
    xb = np.array([[0x00], [0xFF], [0x0F], [0x0F]], dtype=np.uint8)
    xq = np.array([[0x0F], [0x00]], dtype=np.uint8)
    lims, D, I = br.range_search(xb, xq, 0)
    assert lims.tolist() == [0, 0, 0] and D.size == 0 and I.size == 0
    lims, D, I = br.range_search(xb, xq, 1)  # exact duplicates only: the comparison is strict
    assert lims.tolist() == [0, 2, 3] and I.tolist() == [2, 3, 0] and D.tolist() == [0.0, 0.0, 0.0] and D.dtype == np.float32
    lims, D, I = br.range_search(xb, xq, 9)  # d + 1: every row, in row order
    assert lims.tolist() == [0, 4, 8] and I.tolist() == [0, 1, 2, 3] * 2 and D.tolist() == [4, 4, 0, 0, 0, 8, 4, 4]
    lims, D, I = br.range_search(xb, xq, 9, sel=("batch", [3]), id_map=[0, 0, 0, 3])
    assert lims.tolist() == [0, 1, 2] and I.tolist() == [3, 3] and D.tolist() == [0.0, 4.0]


def test_file_round_trip_through_the_python_writer_and_parser():
    rng = np.random.default_rng(3)
    xb = rng.integers(0, 256, (37, 9), dtype=np.uint8)
    im = br.parse_image(br.write_image(xb, 72))
    assert im["kind"] == "IBxF" and im["d"] == 72 and im["ntotal"] == 37 and im["ids"] is None and np.array_equal(im["codes"], xb)
    ids = rng.integers(-5, 1 << 40, 37)
    for two in (False, True):
        im = br.parse_image(br.write_image(xb, 72, id_map=ids, idmap2=two))
        assert im["kind"] == ("IBM2" if two else "IBMp") and np.array_equal(im["codes"], xb) and np.array_equal(im["ids"], ids)
    raw = br.write_image(xb, 72)
    assert raw[:4] == b"IBxF" and len(raw) == 4 + 21 + 8 + 37 * 9
    assert br.parse_image(br.write_image(xb[:0], 72))["ntotal"] == 0


def test_parser_rejects_truncated_and_wrong_size_files():
    xb = np.arange(40, dtype=np.uint8).reshape(5, 8)
    raw = br.write_image(xb, 64, id_map=np.arange(5))
    for cut in (2, 10, 30, 60, len(raw) - 1):
        with pytest.raises(br.ParseError):
            br.parse_image(raw[:cut])
    with pytest.raises(br.ParseError, match="code_size"):
        br.parse_image(br.write_image(xb, 64, code_size=4))
    with pytest.raises(br.ParseError, match="codes hold"):
        br.parse_image(br.write_image(xb, 64, nbytes=39))
    with pytest.raises(br.ParseError, match="fourcc"):
        br.parse_image(b"IxF2" + raw[4:])
    with pytest.raises(br.ParseError):
        br.parse_image(raw + b"\0")
