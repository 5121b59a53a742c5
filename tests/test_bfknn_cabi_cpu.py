"""CPU-side checks of the bfKnn boundary: the header declares mvs_bf_knn and mvs_distance_params and names the contract's phrases, the
built library exports the entry point, the Python host lists it, and the adaptor header declares FAISS's names."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")
ADAPTOR = os.path.join(ROOT, "duckdb-faiss-ext_amd", "compat", "faiss", "gpu", "GpuDistance.h")
FIELDS = ("metric", "k", "dims", "vectors", "vector_type", "vectors_row_major", "num_vectors", "vector_norms", "queries", "query_type",
          "queries_row_major", "num_queries", "out_distances", "ignore_out_distances", "out_indices", "out_indices_type", "device", "stream")


def test_header_declares_the_entry_point_and_the_contract():
    full = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"int\s+mvs_bf_knn\s*\(\s*const\s+mvs_distance_params\s*\*", src)
    body = re.search(r"typedef\s+struct\s+mvs_distance_params\s*\{(.*?)\}\s*mvs_distance_params\s*;", src, flags=re.S).group(1)
    for field in FIELDS:
        assert re.search(r"\b%s\s*;" % field, body), field
    for name in ("MVS_DIST_F32", "MVS_DIST_F16", "MVS_IDX_I64", "MVS_IDX_I32"):
        assert re.search(r"#define\s+%s\s+\d" % name, src), name
    for phrase in ("brute-force k-NN on caller-owned matrices", "never copied when it is f16", "round-to-nearest-even", "k ascending from +0",
                   "used as n_i verbatim", "v_mfma_f32_16x16x32_f16", "max(0, fmaf(-2, s, m_q + n_i))", "bit-identical to a useFloat16 clone",
                   "out_distances[q * num_vectors + i]", "this route costs a copy of the matrix", "1 <= dims <= 2048", "k == -1",
                   "This index type is not implemented on the MI355X path yet: bfKnn", "'k > 0' failed"):
        assert phrase in full, phrase


def test_library_exports_and_python_host_lists_it():
    import mi355_faiss as mf

    assert hasattr(ctypes.CDLL(mf.LIB_PATH), "mvs_bf_knn") and "mvs_bf_knn" in mf.DECLARED_SYMBOLS
    assert [f for f, _ in mf.DistanceParams._fields_] == [
        "metric", "k", "dims", "vectors", "vector_type", "vectors_row_major", "num_vectors", "vector_norms", "queries", "query_type",
        "queries_row_major", "num_queries", "out_distances", "ignore_out_distances", "out_indices_type", "out_indices", "device", "stream",
    ]  # fmt: skip
    assert callable(mf.bf_knn_torch) and callable(mf.bf_knn) and callable(mf.pairwise_distances_torch)


def test_adaptor_header_declares_faiss_names():
    src = open(ADAPTOR).read()
    assert re.search(r"struct\s+GpuDistanceParams\s*\{", src) and re.search(r"void\s+bfKnn\s*\(\s*GpuResourcesProvider\s*\*", src)
    assert "enum class DistanceDataType" in src and "enum class IndicesDataType" in src
    for field in ("vectorsRowMajor", "vectorNorms", "queriesRowMajor", "ignoreOutDistances", "outIndicesType"):
        assert field in src, field
