"""CPU-side checks of the half-precision Flat boundary: the header declares the new entry points and names the contract's phrases, the built
library exports them, and the Python host lists them."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")
FUNCTIONS = ("mvs_index_clone_to_gpu_opts", "mvs_debug_mfma_f16_16x16x32")


def test_header_declares_the_entry_points_and_the_contract():
    full = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in FUNCTIONS:
        assert re.search(r"int\s+%s\s*\(" % name, src), name
    assert re.search(r"typedef\s+struct\s+mvs_cloner_options\s*\{\s*int32_t\s+use_float16\s*;", src)
    assert re.search(r"#define\s+MVS_KIND_FLAT16\s+12\b", src)
    for phrase in ("half-precision Flat", "round-to-nearest-even", "subnormals are kept", "k ascending from +0", "v_mfma_f32_16x16x32_f16",
                   "may depend on d only", "max(0, fmaf(-2, s, m_q + n_i))", "the smaller row wins a tie", "strictly better than +-FLT_MAX",
                   "1 <= d <= 2048", "1 <= k <= 2048", "flat16_device_bytes", "IxF2", "This index type is not implemented on the MI355X path yet"):
        assert phrase in full, phrase


def test_library_exports_and_python_host_lists_them():
    import mi355_faiss as mf

    L = ctypes.CDLL(mf.LIB_PATH)
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in mf.DECLARED_SYMBOLS, name
    assert mf.KIND_FLAT16 == 12 and callable(mf.mfma_f16_16x16x32)
