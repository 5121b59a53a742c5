"""CPU-side checks of the fp16 scalar-quantised inverted lists' boundary: the header declares the new entry points and names the contract's
phrases, the built library exports them, and the Python host lists them."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")
FUNCTIONS = ("mvs_gpu_index_ivfsq_new", "mvs_index_sq_qtype")


def test_header_declares_the_entry_points_and_the_contract():
    full = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in FUNCTIONS:
        assert re.search(r"int\s+%s\s*\(" % name, src), name
    assert re.search(r"#define\s+MVS_QT_8BIT\s+0\b", src) and re.search(r"#define\s+MVS_QT_FP16\s+4\b", src)
    for phrase in ("fp16 scalar-quantised inverted lists", "GpuIndexIVFScalarQuantizer", "index_factory keeps refusing", "There is no range",
                   "round-to-nearest-even", "subnormals are kept", "THE QUERY IS NOT ROUNDED TO fp16", "hi = fp16(v), lo = fp16(v - f32(hi))",
                   "v_mfma_f32_16x16x32_f16", "may depend on d only", "max(0, fmaf(-2, s, m_v + n_h))", "whatever other pairs share its pair group",
                   "(score, probe rank, position in the list)", "1 <= d <= 2048", "code_size 2 d", "sqfp16_scan_kernel"):
        assert phrase in full, phrase


def test_library_exports_and_python_host_lists_them():
    import mi355_faiss as mf

    L = ctypes.CDLL(mf.LIB_PATH)
    for name in FUNCTIONS:
        assert hasattr(L, name), name
        assert name in mf.DECLARED_SYMBOLS, name
    assert (mf.QT_8bit, mf.QT_fp16) == (0, 4) and callable(mf.GpuIndexIVFScalarQuantizer) and isinstance(mf.Index.sq_qtype, property)
