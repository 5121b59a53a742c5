"""ctypes host binding of libmi355faiss.so (include/mi355_faiss.h).

Mirrors the faiss.Index surface the reference DuckDB extension reaches from
/root/reference/src/faiss_extension.cpp (:154 index_factory, :396/:583 train, :510/:607
add_with_ids, :512/:609 add, :631 search, gpu.cpp:48 index_cpu_to_gpu) with the same names,
argument meaning and error text, so the parity tests read like the reference's tests.

There is NO CPU fallback: if the HIP library is missing this module raises at import, and
every call fails loudly when no gfx950 device is usable.
"""
import ctypes as C
import os
import sys

import numpy as np

METRIC_INNER_PRODUCT = 0
METRIC_L2 = 1
KIND_FLAT, KIND_IDMAP, KIND_IVFFLAT, KIND_HNSW, KIND_PQ, KIND_IVFPQ, KIND_SQ, KIND_IVFSQ, KIND_HNSWSQ, KIND_REFINE = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
KIND_PRETRANSFORM = 11
VT_LINEAR, VT_PCA, VT_NORM = 0, 1, 2
SEL_NONE, SEL_BITMAP, SEL_BATCH = 0, 1, 2

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MVS_LIB_PATH") or os.path.join(_PKG, "libmi355faiss.so")  # (override: A/B of two builds)


class FaissException(RuntimeError):
    """faiss::FaissException -- .msg carries the text the reference greps (src/faiss_extension.cpp:400,523,592)"""

    @property
    def msg(self):
        return self.args[0]


class SearchParams(C.Structure):
    _fields_ = [
        ("nprobe", C.c_int64),
        ("efSearch", C.c_int64),
        ("sel_kind", C.c_int32),
        ("reserved", C.c_int32),
        ("sel_data", C.c_void_p),
        ("sel_n", C.c_int64),
    ]


class KernelInfo(C.Structure):
    _fields_ = [
        ("name", C.c_char * 64),
        ("flops", C.c_double),
        ("bytes", C.c_double),
        ("last_ms", C.c_double),
        ("grid", C.c_int32),
        ("block", C.c_int32),
        ("lds_bytes", C.c_int32),
        ("nsplit", C.c_int32),
    ]


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950); the MI355X vector-search path has no CPU fallback"
    )


def _preload_hip_runtime():
    """libmi355faiss.so is linked without a NEEDED entry for libamdhip64 (csrc/Makefile): the host picks the
    HIP runtime.  PyTorch wheels bundle their own libamdhip64 + libhsa-runtime64, and two HSA runtimes cannot
    coexist in one process, so when torch is installed its copy is the one to share."""
    import importlib.util

    cands = []
    spec = importlib.util.find_spec("torch")
    if spec and spec.submodule_search_locations:
        cands.append(os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so"))
    cands += ["/opt/rocm/lib/libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so"]
    errs = []
    for c in cands:
        if os.path.isabs(c) and not os.path.exists(c):
            continue
        try:
            return C.CDLL(c, mode=C.RTLD_GLOBAL)
        except OSError as e:  # pragma: no cover
            errs.append(f"{c}: {e}")
    raise ImportError("no HIP runtime (libamdhip64) could be loaded: " + "; ".join(errs))


_HIP = _preload_hip_runtime()
_L = C.CDLL(LIB_PATH)
_p, _i64 = C.c_void_p, C.c_int64
_L.mvs_last_error.restype = C.c_char_p
_L.mvs_version.restype = C.c_char_p
_L.mvs_index_factory.argtypes = [C.POINTER(_p), C.c_int, C.c_char_p, C.c_int]
_L.mvs_index_free.argtypes = [_p]
_L.mvs_index_d.argtypes = [_p]
_L.mvs_index_ntotal.argtypes = [_p]
_L.mvs_index_ntotal.restype = _i64
_L.mvs_index_is_trained.argtypes = [_p]
_L.mvs_index_metric_type.argtypes = [_p]
_L.mvs_index_kind.argtypes = [_p]
_L.mvs_index_device.argtypes = [_p]
_L.mvs_index_idmap_sub.argtypes = [_p]
_L.mvs_index_idmap_sub.restype = _p
_L.mvs_index_ivf_quantizer.argtypes = [_p]
_L.mvs_index_ivf_quantizer.restype = _p
_L.mvs_index_hnsw_set_ef_construction.argtypes = [_p, C.c_int]
_L.mvs_index_hnsw_get_ef_construction.argtypes = [_p]
_L.mvs_index_hnsw_graph_info.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
_L.mvs_index_hnsw_graph_info.restype = _i64
_L.mvs_index_hnsw_walk_stats.argtypes = [_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
_L.mvs_index_hnsw_get_graph.argtypes = [_p, _p, _p, _p]
_L.mvs_index_ivf_nlist.argtypes = [_p]
_L.mvs_index_ivf_nlist.restype = _i64
_L.mvs_index_ivf_get_centroids.argtypes = [_p, _p]
_L.mvs_index_ivf_set_centroids.argtypes = [_p, _p]
_L.mvs_index_pq_info.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
_L.mvs_index_pq_get_centroids.argtypes = [_p, _p]
_L.mvs_index_pq_set_centroids.argtypes = [_p, _p]
_L.mvs_index_pq_get_codes.argtypes = [_p, _i64, _i64, _p]
_L.mvs_index_ivfpq_list_size.argtypes = [_p, _i64]
_L.mvs_index_ivfpq_list_size.restype = _i64
_L.mvs_index_ivfpq_get_list.argtypes = [_p, _i64, _p, _p]
_L.mvs_index_sq_get_trained.argtypes = [_p, _p]
_L.mvs_index_sq_set_trained.argtypes = [_p, _p]
_L.mvs_index_sq_get_codes.argtypes = [_p, _i64, _i64, _p]
_L.mvs_index_ivfsq_list_size.argtypes = [_p, _i64]
_L.mvs_index_ivfsq_list_size.restype = _i64
_L.mvs_index_ivfsq_get_list.argtypes = [_p, _i64, _p, _p]
_L.mvs_index_refine_base.argtypes = [_p]
_L.mvs_index_refine_base.restype = _p
_L.mvs_index_refine_store.argtypes = [_p]
_L.mvs_index_refine_store.restype = _p
_L.mvs_index_refine_set_k_factor.argtypes = [_p, C.c_float]
_L.mvs_index_refine_get_k_factor.argtypes = [_p, C.POINTER(C.c_float)]
_L.mvs_index_pretransform_sub.argtypes = [_p]
_L.mvs_index_pretransform_sub.restype = _p
_L.mvs_index_pretransform_count.argtypes = [_p]
_L.mvs_index_pretransform_info.argtypes = [_p, C.c_int] + [C.POINTER(C.c_int)] * 5
_L.mvs_index_pretransform_get_linear.argtypes = [_p, C.c_int, _p, _p]
_L.mvs_index_pretransform_set_linear.argtypes = [_p, C.c_int, _p, _p]
_L.mvs_index_pretransform_get_pca.argtypes = [_p, C.c_int, _p, _p]
_L.mvs_index_pretransform_apply.argtypes = [_p, _i64, _p, _p]
_L.mvs_index_pretransform_apply_device.argtypes = [_p, _i64, _p, _p, _p]
_L.mvs_index_train.argtypes = [_p, _i64, _p]
_L.mvs_index_add.argtypes = [_p, _i64, _p]
_L.mvs_index_add_with_ids.argtypes = [_p, _i64, _p, _p]
_L.mvs_index_search.argtypes = [_p, _i64, _p, _i64, _p, _p, C.POINTER(SearchParams)]
_L.mvs_index_range_search.argtypes = [_p, _i64, _p, C.c_float, C.POINTER(SearchParams), C.POINTER(_p)]
_L.mvs_index_remove_ids.argtypes = [_p, C.c_int32, _p, _i64, C.POINTER(_i64)]
_L.mvs_index_merge_from.argtypes = [_p, _p, _i64]
_L.mvs_index_check_compatible_for_merge.argtypes = [_p, _p]
_L.mvs_index_ivf_copy_subset_to.argtypes = [_p, _p, C.c_int, _i64, _i64]
_L.mvs_index_reconstruct.argtypes = [_p, _i64, _p]
_L.mvs_index_reconstruct_n.argtypes = [_p, _i64, _i64, _p]
_L.mvs_index_reconstruct_batch.argtypes = [_p, _i64, _p, _p]
_L.mvs_index_search_and_reconstruct.argtypes = [_p, _i64, _p, _i64, _p, _p, _p, C.POINTER(SearchParams)]
_L.mvs_index_reconstruct_batch_device.argtypes = [_p, _i64, _p, _p, _p]
_L.mvs_index_search_and_reconstruct_device.argtypes = [_p, _i64, _p, _i64, _p, _p, _p, C.POINTER(SearchParams), _p]
_L.mvs_range_result_nq.argtypes = [_p]
_L.mvs_range_result_nq.restype = _i64
_L.mvs_range_result_lims.argtypes = [_p]
_L.mvs_range_result_lims.restype = C.POINTER(_i64)
_L.mvs_range_result_distances.argtypes = [_p]
_L.mvs_range_result_distances.restype = C.POINTER(C.c_float)
_L.mvs_range_result_labels.argtypes = [_p]
_L.mvs_range_result_labels.restype = C.POINTER(_i64)
_L.mvs_range_result_free.argtypes = [_p]
_L.mvs_range_result_free.restype = None
_L.mvs_index_to_gpu.argtypes = [_p, C.c_int]
_L.mvs_index_clone_to_gpu.argtypes = [C.POINTER(_p), _p, C.c_int]
_L.mvs_index_prefilter_stats.argtypes = [_p, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(C.c_float), C.POINTER(C.c_float)]
_L.mvs_index_collect_stats.argtypes = [_p, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]
_L.mvs_index_ivf_probe_stats.argtypes = [_p, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]
_L.mvs_index_shadow_stats.argtypes = [_p, C.POINTER(_i64), C.POINTER(C.c_double)]
_L.mvs_index_get_stat.argtypes = [_p, C.c_char_p, C.POINTER(_i64)]
_L.mvs_trace_push.argtypes = [C.c_char_p]
_L.mvs_trace_pop.argtypes = []
_L.mvs_index_shard_to_gpus.argtypes = [_p, C.POINTER(C.c_int), C.c_int]
_L.mvs_index_shard_info.argtypes = [_p, C.POINTER(C.c_int), C.c_int, C.POINTER(_i64), C.POINTER(_i64)]
_L.mvs_write_index.argtypes = [_p, C.c_char_p]
_L.mvs_read_index.argtypes = [C.POINTER(_p), C.c_char_p]
_L.mvs_index_add_device.argtypes = [_p, _i64, _p, _p, _p]
_L.mvs_index_search_device.argtypes = [_p, _i64, _p, _i64, _p, _p, C.POINTER(SearchParams), _p]
_L.mvs_index_set_label_offset.argtypes = [_p, _i64]
_L.mvs_merge_shards.argtypes = [C.c_int, _i64, _i64, C.c_int, _p, _p, _p, _p]
_L.mvs_merge_shards_raw.argtypes = [C.c_int, _i64, _i64, C.c_int, _p, _p, _p, _p]
_L.mvs_merge_records_device.argtypes = [C.c_int, _i64, C.c_int, C.c_int, C.c_int, _p, C.c_int, _p, _p, _p]
_L.mvs_finish_ip_ties.argtypes = [_i64, _i64, _i64, _p, _p, _i64, _p, _p, _p, _p]
_L.mvs_index_tie_candidates_device.argtypes = [_p, _i64, _p, _p, _i64, _p, C.POINTER(SearchParams), _p]
_L.mvs_index_ivf_tie_emit_device.argtypes = [_p, _i64, _p, _p, _p, _i64, _p, _p, _p, C.POINTER(SearchParams), _p]
_L.mvs_synth_uniform_device.argtypes = [_p, _i64, C.c_int, C.c_uint64, _i64, _p]
_L.mvs_debug_mfma_bf16_16x16x32.argtypes = [_p, _p, _p, _p, _i64]
_L.mvs_synth_clustered_device.argtypes = [_p, _i64, C.c_int, C.c_uint64, _i64, C.c_int, C.c_float, _p]
_L.mvs_index_last_kernel_info.argtypes = [_p, C.POINTER(KernelInfo)]
_L.mvs_index_set_kernel_timing.argtypes = [_p, C.c_int]
_L.mvs_index_kernel_time_stats.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
_L.mvs_index_set_option.argtypes = [_p, C.c_char_p, _i64]
# binary indexes (include/mi355_faiss.h "binary indexes"): a handle type of their own
_L.mvs_binary_index_factory.argtypes = [C.POINTER(_p), C.c_int, C.c_char_p]
_L.mvs_binary_index_free.argtypes = [_p]
_L.mvs_binary_index_free.restype = None
_L.mvs_binary_index_d.argtypes = [_p]
_L.mvs_binary_index_code_size.argtypes = [_p]
_L.mvs_binary_index_ntotal.argtypes = [_p]
_L.mvs_binary_index_ntotal.restype = _i64
_L.mvs_binary_index_kind.argtypes = [_p]
_L.mvs_binary_index_idmap_sub.argtypes = [_p]
_L.mvs_binary_index_idmap_sub.restype = _p
_L.mvs_binary_index_add.argtypes = [_p, _i64, _p]
_L.mvs_binary_index_add_with_ids.argtypes = [_p, _i64, _p, _p]
_L.mvs_binary_index_search.argtypes = [_p, _i64, _p, _i64, _p, _p, C.POINTER(SearchParams)]
_L.mvs_binary_index_range_search.argtypes = [_p, _i64, _p, C.c_int, C.POINTER(SearchParams), C.POINTER(_p)]
_L.mvs_binary_index_reset.argtypes = [_p]
_L.mvs_binary_index_reconstruct.argtypes = [_p, _i64, _p]
_L.mvs_binary_index_reconstruct_n.argtypes = [_p, _i64, _i64, _p]
_L.mvs_binary_index_add_device.argtypes = [_p, _i64, _p, _p, _p]
_L.mvs_binary_index_search_device.argtypes = [_p, _i64, _p, _i64, _p, _p, C.POINTER(SearchParams), _p]
_L.mvs_binary_index_set_option.argtypes = [_p, C.c_char_p, _i64]
_L.mvs_binary_index_get_stat.argtypes = [_p, C.c_char_p, C.POINTER(_i64)]
_L.mvs_write_index_binary.argtypes = [_p, C.c_char_p]
_L.mvs_read_index_binary.argtypes = [C.POINTER(_p), C.c_char_p]

# every symbol include/mi355_faiss.h declares (tests check the library exports all of them)
DECLARED_SYMBOLS = [
    "mvs_last_error", "mvs_index_factory", "mvs_index_free", "mvs_index_d", "mvs_index_ntotal",
    "mvs_index_is_trained", "mvs_index_metric_type", "mvs_index_kind", "mvs_index_idmap_sub",
    "mvs_index_ivf_quantizer", "mvs_index_ivf_nlist", "mvs_index_ivf_get_centroids", "mvs_index_ivf_set_centroids",
    "mvs_index_hnsw_set_ef_construction", "mvs_index_hnsw_get_ef_construction", "mvs_index_hnsw_graph_info", "mvs_index_hnsw_walk_stats", "mvs_index_hnsw_get_graph",
    "mvs_index_pq_info", "mvs_index_pq_get_centroids", "mvs_index_pq_set_centroids", "mvs_index_pq_get_codes",
    "mvs_index_ivfpq_list_size", "mvs_index_ivfpq_get_list",
    "mvs_index_sq_get_trained", "mvs_index_sq_set_trained", "mvs_index_sq_get_codes", "mvs_index_ivfsq_list_size", "mvs_index_ivfsq_get_list",
    "mvs_index_refine_base", "mvs_index_refine_store", "mvs_index_refine_set_k_factor", "mvs_index_refine_get_k_factor",
    "mvs_index_pretransform_sub", "mvs_index_pretransform_count", "mvs_index_pretransform_info", "mvs_index_pretransform_get_linear",
    "mvs_index_pretransform_set_linear", "mvs_index_pretransform_get_pca", "mvs_index_pretransform_apply", "mvs_index_pretransform_apply_device",
    "mvs_index_train", "mvs_index_add",
    "mvs_index_add_with_ids", "mvs_index_search",
    "mvs_index_remove_ids",
    "mvs_index_merge_from", "mvs_index_check_compatible_for_merge", "mvs_index_ivf_copy_subset_to",
    "mvs_index_reconstruct", "mvs_index_reconstruct_n", "mvs_index_reconstruct_batch", "mvs_index_search_and_reconstruct",
    "mvs_index_reconstruct_batch_device", "mvs_index_search_and_reconstruct_device",
    "mvs_index_range_search", "mvs_range_result_nq", "mvs_range_result_lims", "mvs_range_result_distances", "mvs_range_result_labels", "mvs_range_result_free",
    "mvs_index_to_gpu", "mvs_index_device", "mvs_index_clone_to_gpu",
    "mvs_index_prefilter_stats", "mvs_index_collect_stats", "mvs_index_ivf_probe_stats", "mvs_index_shadow_stats", "mvs_index_get_stat", "mvs_trace_push", "mvs_trace_pop", "mvs_index_shard_to_gpus", "mvs_index_shard_info", "mvs_write_index",
    "mvs_read_index", "mvs_index_add_device", "mvs_index_search_device", "mvs_index_set_label_offset",
    "mvs_merge_shards", "mvs_merge_shards_raw", "mvs_merge_records_device", "mvs_finish_ip_ties", "mvs_index_tie_candidates_device", "mvs_index_ivf_tie_emit_device", "mvs_synth_uniform_device", "mvs_synth_clustered_device", "mvs_debug_mfma_bf16_16x16x32", "mvs_index_last_kernel_info",
    "mvs_index_set_kernel_timing", "mvs_index_kernel_time_stats", "mvs_index_set_option", "mvs_device_count",
    "mvs_version",
    "mvs_binary_index_factory", "mvs_binary_index_free", "mvs_binary_index_d", "mvs_binary_index_code_size", "mvs_binary_index_ntotal",
    "mvs_binary_index_kind", "mvs_binary_index_idmap_sub", "mvs_binary_index_add", "mvs_binary_index_add_with_ids", "mvs_binary_index_search",
    "mvs_binary_index_range_search", "mvs_binary_index_reset", "mvs_binary_index_reconstruct", "mvs_binary_index_reconstruct_n",
    "mvs_binary_index_add_device", "mvs_binary_index_search_device", "mvs_binary_index_set_option", "mvs_binary_index_get_stat",
    "mvs_write_index_binary", "mvs_read_index_binary",
]  # fmt: skip


def lib():
    return _L


class trace_range:
    """with trace_range("exchange"): ... -- a roctx range (include/mi355_faiss.h mvs_trace_push / mvs_trace_pop)"""

    def __init__(self, name):
        self.name = name.encode()

    def __enter__(self):
        _L.mvs_trace_push(self.name)
        return self

    def __exit__(self, *exc):
        _L.mvs_trace_pop()
        return False


def _check(rc):
    if rc:
        raise FaissException(_L.mvs_last_error().decode())


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i64a(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class SelNode(C.Structure):
    """mvs_sel_node: one node of a selector program (include/mi355_faiss.h "selector programs")"""

    _fields_ = [
        ("op", C.c_int32),
        ("reserved", C.c_int32),
        ("data", C.c_void_p),
        ("n", C.c_int64),
        ("imin", C.c_int64),
        ("imax", C.c_int64),
    ]


SEL_PROGRAM = 3
SELOP_ALL, SELOP_BITMAP, SELOP_BATCH, SELOP_ARRAY, SELOP_RANGE, SELOP_NOT, SELOP_AND, SELOP_OR, SELOP_XOR = range(1, 10)
_SEL_LEAF_IDS = {"batch": SELOP_BATCH, "array": SELOP_ARRAY}
_SEL_BINARY = {"and": SELOP_AND, "or": SELOP_OR, "xor": SELOP_XOR}


def _flatten_selector(tree, nodes, keep):
    """nested tuples -> postfix nodes (op, array or None, imin, imax); `keep` collects the arrays the nodes point into"""
    kind = tree[0]
    if kind == "all" and len(tree) == 1:
        nodes.append((SELOP_ALL, None, 0, 0))
    elif kind == "range" and len(tree) == 3:
        nodes.append((SELOP_RANGE, None, int(tree[1]), int(tree[2])))
    elif kind == "bitmap" and len(tree) == 2:
        a = np.ascontiguousarray(tree[1], dtype=np.uint8)
        keep.append(a)
        nodes.append((SELOP_BITMAP, a, 0, 0))
    elif kind in _SEL_LEAF_IDS and len(tree) == 2:
        a = _i64a(tree[1])
        keep.append(a)
        nodes.append((_SEL_LEAF_IDS[kind], a, 0, 0))
    elif kind == "not" and len(tree) == 2:
        _flatten_selector(tree[1], nodes, keep)
        nodes.append((SELOP_NOT, None, 0, 0))
    elif kind in _SEL_BINARY and len(tree) == 3:
        _flatten_selector(tree[1], nodes, keep)
        _flatten_selector(tree[2], nodes, keep)
        nodes.append((_SEL_BINARY[kind], None, 0, 0))
    else:
        raise ValueError("selector %r" % (tree,))


def make_params(nprobe=0, efSearch=0, sel=None):
    """sel: None | ("bitmap", uint8 array) | ("batch", int64 array) -- IDSelectorBitmap / IDSelectorBatch, as MVS_SEL_BITMAP / MVS_SEL_BATCH;
    or a tree of ("range", a, b) | ("array", ids) | ("all",) | ("not", s) | ("and", s, t) | ("or", s, t) | ("xor", s, t) with ("bitmap", a) /
    ("batch", a) as leaves -- IDSelectorRange / Array / All / Not / And / Or / XOr, as MVS_SEL_PROGRAM; or ("program", nodes) with nodes a
    list of (op, array or None, imin, imax[, n]) handed over as they are.  The second value keeps the selector's memory alive."""
    p = SearchParams()
    p.nprobe, p.efSearch = nprobe, efSearch
    keep = None
    if sel is not None:
        kind = sel[0]
        if kind == "bitmap" and len(sel) == 2:
            keep = np.ascontiguousarray(sel[1], dtype=np.uint8)
            p.sel_kind = SEL_BITMAP
        elif kind == "batch" and len(sel) == 2:
            keep = _i64a(sel[1])
            p.sel_kind = SEL_BATCH
        else:
            nodes, arrays = [], []
            if kind == "program":
                nodes = list(sel[1])
            else:
                _flatten_selector(sel, nodes, arrays)
            arr = (SelNode * max(len(nodes), 1))()
            for i, nd in enumerate(nodes):
                op, a, imin, imax = nd[:4]
                arr[i].op, arr[i].imin, arr[i].imax = op, imin, imax
                arr[i].data = a.ctypes.data if a is not None else None
                arr[i].n = nd[4] if len(nd) > 4 else (a.size if a is not None else 0)
            p.sel_kind = SEL_PROGRAM
            p.sel_n = len(nodes)
            p.sel_data = C.cast(arr, C.c_void_p).value
            return p, (arr, arrays, nodes)
        p.sel_n = keep.size
        p.sel_data = keep.ctypes.data
    return p, keep


def device_count():
    return _L.mvs_device_count()


class Index:
    """Device-native index; same method names as faiss.Index."""

    def __init__(self, handle, owned=True, parent=None):
        self._h = handle
        self._owned = owned
        self._parent = parent  # keeps the owning index alive for borrowed handles

    def __del__(self, _free=_L.mvs_index_free, _finalizing=sys.is_finalizing):
        # (both bound at definition: module globals are None during interpreter shutdown.  Indexes still alive when the interpreter
        # finalizes are NOT freed: the HIP runtime / RCCL may already be gone -- freeing a sharded index then aborted the process with
        # "double free or corruption" after the test summary; the OS reclaims the device memory with the process)
        if getattr(self, "_h", None) and getattr(self, "_owned", False) and not _finalizing():
            _free(self._h)
        self._h = None

    d = property(lambda s: _L.mvs_index_d(s._h))
    ntotal = property(lambda s: _L.mvs_index_ntotal(s._h))
    is_trained = property(lambda s: bool(_L.mvs_index_is_trained(s._h)))
    metric_type = property(lambda s: _L.mvs_index_metric_type(s._h))
    kind = property(lambda s: _L.mvs_index_kind(s._h))
    device = property(lambda s: _L.mvs_index_device(s._h))

    @property
    def index(self):
        """IndexIDMap::index (src/faiss_extension.cpp:129)"""
        h = _L.mvs_index_idmap_sub(self._h)
        return Index(h, owned=False, parent=self) if h else None

    @property
    def quantizer(self):
        """IndexIVF::quantizer (src/faiss_extension.cpp:680)"""
        h = _L.mvs_index_ivf_quantizer(self._h)
        return Index(h, owned=False, parent=self) if h else None

    @property
    def nlist(self):
        return _L.mvs_index_ivf_nlist(self._h)

    def ivf_centroids(self):
        out = np.empty((self.nlist, self.d), dtype=np.float32)
        _check(_L.mvs_index_ivf_get_centroids(self._h, _ptr(out)))
        return out

    def ivf_set_centroids(self, c):
        c = _f32(c).reshape(self.nlist, self.d)
        _check(_L.mvs_index_ivf_set_centroids(self._h, _ptr(c)))

    def pq_info(self):
        """-> (M, nbits) of a PQ<M> index (IDMap wrappers are looked through) -- include/mi355_faiss.h mvs_index_pq_info"""
        M, nbits = C.c_int(0), C.c_int(0)
        _check(_L.mvs_index_pq_info(self._h, C.byref(M), C.byref(nbits)))
        return M.value, nbits.value

    def pq_centroids(self):
        """the codebooks, [M, 256, d / M]"""
        M, _ = self.pq_info()
        out = np.empty((M, 256, self.d // M), dtype=np.float32)
        _check(_L.mvs_index_pq_get_centroids(self._h, _ptr(out)))
        return out

    def pq_set_centroids(self, c):
        """install codebooks [M, 256, d / M] and mark the index trained (only while it is empty)"""
        M, _ = self.pq_info()
        c = _f32(c).reshape(M, 256, self.d // M)
        _check(_L.mvs_index_pq_set_centroids(self._h, _ptr(c)))

    def pq_codes(self, row0=0, n=None):
        """code bytes of rows [row0, row0 + n), [n, M] uint8"""
        M, _ = self.pq_info()
        n = self.ntotal - row0 if n is None else n
        out = np.empty((max(n, 0), M), dtype=np.uint8)
        _check(_L.mvs_index_pq_get_codes(self._h, row0, n, _ptr(out)))
        return out

    def ivfpq_list_size(self, list_no):
        """rows of inverted list list_no of an IVF<n>,PQ<M> index (IDMap wrappers are looked through)"""
        n = _L.mvs_index_ivfpq_list_size(self._h, int(list_no))
        if n < 0:
            raise FaissException(_L.mvs_last_error().decode())
        return n

    def ivfpq_list(self, list_no):
        """-> (stored ids [n] int64, codes [n, M] uint8) of inverted list list_no, in list order"""
        M, _ = self.pq_info()
        n = self.ivfpq_list_size(list_no)
        ids, codes = np.empty(n, dtype=np.int64), np.empty((n, M), dtype=np.uint8)
        _check(_L.mvs_index_ivfpq_get_list(self._h, int(list_no), _ptr(ids), _ptr(codes)))
        return ids, codes

    def sq_trained(self):
        """-> (vmin [d], vdiff [d]) of an SQ8 / IVF<n>,SQ8 / HNSW<M>,SQ8 index (IDMap wrappers are looked through) -- mvs_index_sq_get_trained"""
        out = np.empty((2, self.d), dtype=np.float32)
        _check(_L.mvs_index_sq_get_trained(self._h, _ptr(out)))
        return out[0].copy(), out[1].copy()

    def sq_set_trained(self, vmin, vdiff):
        """install the range and mark the index trained (IVF<n>,SQ8: once the centroids are present too); only while it is empty"""
        t = np.concatenate([_f32(vmin).reshape(self.d), _f32(vdiff).reshape(self.d)])
        _check(_L.mvs_index_sq_set_trained(self._h, _ptr(t)))

    def sq_codes(self, row0=0, n=None):
        """code bytes of rows [row0, row0 + n) of an SQ8 index (HNSW<M>,SQ8: in vertex order), [n, d] uint8"""
        n = self.ntotal - row0 if n is None else n
        out = np.empty((max(n, 0), self.d), dtype=np.uint8)
        _check(_L.mvs_index_sq_get_codes(self._h, row0, n, _ptr(out)))
        return out

    def ivfsq_list_size(self, list_no):
        """rows of inverted list list_no of an IVF<n>,SQ8 index (IDMap wrappers are looked through)"""
        n = _L.mvs_index_ivfsq_list_size(self._h, int(list_no))
        if n < 0:
            raise FaissException(_L.mvs_last_error().decode())
        return n

    def ivfsq_list(self, list_no):
        """-> (stored ids [n] int64, codes [n, d] uint8) of inverted list list_no, in list order"""
        n = self.ivfsq_list_size(list_no)
        ids, codes = np.empty(n, dtype=np.int64), np.empty((n, self.d), dtype=np.uint8)
        _check(_L.mvs_index_ivfsq_get_list(self._h, int(list_no), _ptr(ids), _ptr(codes)))
        return ids, codes

    @property
    def refine_base(self):
        """IndexRefine::base_index of a "<base>,RFlat" index (IDMap wrappers are looked through); None on another kind.  The pq_* / ivf_* /
        sq_* accessors take this handle"""
        h = _L.mvs_index_refine_base(self._h)
        return Index(h, owned=False, parent=self) if h else None

    @property
    def refine_store(self):
        """IndexRefine::refine_index: the Flat index holding the rows in arrival order; None on another kind"""
        h = _L.mvs_index_refine_store(self._h)
        return Index(h, owned=False, parent=self) if h else None

    @property
    def k_factor(self):
        """IndexRefine::k_factor: the base index is asked for (int64)((float)k * k_factor) candidates"""
        v = C.c_float(0)
        _check(_L.mvs_index_refine_get_k_factor(self._h, C.byref(v)))
        return v.value

    @k_factor.setter
    def k_factor(self, v):
        _check(_L.mvs_index_refine_set_k_factor(self._h, C.c_float(float(v))))

    # ---- pre-transform indexes (include/mi355_faiss.h "pre-transform indexes"); IDMap wrappers are looked through
    @property
    def pretransform_sub(self):
        """IndexPreTransform::index of a "<t1>,...,<sub>" index; None on another kind.  The ivf_* / pq_* / sq_* accessors take this handle"""
        h = _L.mvs_index_pretransform_sub(self._h)
        return Index(h, owned=False, parent=self) if h else None

    @property
    def pretransform_count(self):
        """IndexPreTransform::chain.size(); -1 on another kind"""
        return _L.mvs_index_pretransform_count(self._h)

    def pretransform_info(self, i):
        """-> dict(type=VT_*, d_in, d_out, have_bias, is_trained) of transform i"""
        v = [C.c_int(0) for _ in range(5)]
        _check(_L.mvs_index_pretransform_info(self._h, int(i), *[C.byref(e) for e in v]))
        return dict(type=v[0].value, d_in=v[1].value, d_out=v[2].value, have_bias=bool(v[3].value), is_trained=bool(v[4].value))

    def pretransform_get_linear(self, i):
        """-> (A [d_out, d_in], b [d_out]) of a trained linear or PCA transform; b is zeros without a bias"""
        t = self.pretransform_info(i)
        A, b = np.empty((t["d_out"], t["d_in"]), dtype=np.float32), np.empty(t["d_out"], dtype=np.float32)
        _check(_L.mvs_index_pretransform_get_linear(self._h, int(i), _ptr(A), _ptr(b)))
        return A, b

    def pretransform_set_linear(self, i, A, b=None):
        """install A [d_out, d_in] and b [d_out] (None: no bias), mark the transform trained; only while the index is empty"""
        t = self.pretransform_info(i)
        A = _f32(A).reshape(t["d_out"], t["d_in"])
        b = None if b is None else _f32(b).reshape(t["d_out"])
        _check(_L.mvs_index_pretransform_set_linear(self._h, int(i), _ptr(A), _ptr(b) if b is not None else None))

    def pretransform_get_pca(self, i):
        """-> (mean [d_in], eigenvalues [d_in]) of a trained PCA transform"""
        t = self.pretransform_info(i)
        mean, ev = np.empty(t["d_in"], dtype=np.float32), np.empty(t["d_in"], dtype=np.float32)
        _check(_L.mvs_index_pretransform_get_pca(self._h, int(i), _ptr(mean), _ptr(ev)))
        return mean, ev

    def pretransform_apply(self, x):
        """IndexPreTransform::apply_chain -> [n, d_out of the chain] float32"""
        x = _f32(x).reshape(-1, self.d)
        dout = self.pretransform_info(self.pretransform_count - 1)["d_out"]
        out = np.empty((x.shape[0], dout), dtype=np.float32)
        _check(_L.mvs_index_pretransform_apply(self._h, x.shape[0], _ptr(x), _ptr(out)))
        return out

    def pretransform_apply_torch(self, x, out=None, stream=None):
        """the same on a float32 tensor on the index's device (mvs_index_pretransform_apply_device)"""
        import torch

        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        dout = self.pretransform_info(self.pretransform_count - 1)["d_out"]
        if out is None:
            out = torch.empty((x.shape[0], dout), dtype=torch.float32, device=x.device)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(_L.mvs_index_pretransform_apply_device(self._h, x.shape[0], x.data_ptr(), out.data_ptr(), stream))
        return out

    def set_ef_construction(self, v):
        _check(_L.mvs_index_hnsw_set_ef_construction(self._h, int(v)))

    def hnsw_walk_stats(self):
        """counters of the last search run with kernel timing on: distance evaluations, f32 rows fetched (HNSW<M>,SQ8: code rows), bf16 rows
        looked at (HNSW<M>,SQ8: 0)"""
        ev, f32, bf = C.c_double(), C.c_double(), C.c_double()
        _check(_L.mvs_index_hnsw_walk_stats(self._h, C.byref(ev), C.byref(f32), C.byref(bf)))
        return {"evaluations": ev.value, "f32_rows": f32.value, "bf16_rows": bf.value}

    def hnsw_graph(self):
        """-> dict(levels[n], offsets[n+1], neighbors[...], max_level, entry_point) (FAISS's HNSW arrays)"""
        ml, ep = C.c_int(0), C.c_int(0)
        nb = _L.mvs_index_hnsw_graph_info(self._h, C.byref(ml), C.byref(ep))
        if nb < 0:
            raise FaissException("not an HNSW index")
        n = self.ntotal
        levels = np.empty(n, dtype=np.int32)
        offsets = np.empty(n + 1, dtype=np.int64)
        neighbors = np.empty(max(nb, 1), dtype=np.int32)
        _check(_L.mvs_index_hnsw_get_graph(self._h, _ptr(levels), _ptr(offsets), _ptr(neighbors)))
        return dict(levels=levels, offsets=offsets, neighbors=neighbors[:nb], max_level=ml.value, entry_point=ep.value)

    def train(self, x):
        x = _f32(x).reshape(-1, self.d)
        _check(_L.mvs_index_train(self._h, x.shape[0], _ptr(x)))

    def add(self, x):
        x = _f32(x).reshape(-1, self.d)
        _check(_L.mvs_index_add(self._h, x.shape[0], _ptr(x)))

    def add_with_ids(self, x, ids):
        x = _f32(x).reshape(-1, self.d)
        ids = _i64a(ids)
        assert ids.size == x.shape[0]
        _check(_L.mvs_index_add_with_ids(self._h, x.shape[0], _ptr(x), _ptr(ids)))

    def search(self, x, k, nprobe=0, efSearch=0, sel=None):
        x = _f32(x).reshape(-1, self.d)
        nq = x.shape[0]
        D = np.empty((nq, max(k, 0)), dtype=np.float32)
        I = np.empty((nq, max(k, 0)), dtype=np.int64)
        p, keep = make_params(nprobe, efSearch, sel)
        _check(_L.mvs_index_search(self._h, nq, _ptr(x), k, _ptr(D), _ptr(I), C.byref(p)))
        del keep
        return D, I

    def remove_ids(self, sel):
        """faiss::Index::remove_ids: the rows whose id is a member of `sel` go; returns their number.  sel as for search:
        ("bitmap", uint8 array) | ("batch", int64 array) (include/mi355_faiss.h "remove_ids")"""
        p, keep = make_params(0, 0, sel)
        n = _i64(0)
        _check(_L.mvs_index_remove_ids(self._h, p.sel_kind, C.c_void_p(p.sel_data), p.sel_n, C.byref(n)))
        return int(n.value)

    # ---- merge_from and copy_subset_to (include/mi355_faiss.h "merge_from and copy_subset_to"): rows move between indexes on the device
    SUBSET_TYPE_ID_RANGE, SUBSET_TYPE_ID_MOD, SUBSET_TYPE_ELEMENT_RANGE = 0, 1, 2

    def merge_from(self, other, add_id=0):
        """faiss.Index.merge_from: other's rows follow this index's (an IVF kind: stored id + add_id); other ends empty but trained"""
        _check(_L.mvs_index_merge_from(self._h, other._h, int(add_id)))

    def check_compatible_for_merge(self, other):
        """faiss.Index.check_compatible_for_merge: raises with the first difference; changes nothing"""
        _check(_L.mvs_index_check_compatible_for_merge(self._h, other._h))

    def copy_subset_to(self, other, subset_type, a1, a2):
        """faiss.IndexIVF.copy_subset_to (the bare IVF kinds): the entries a subset type selects are appended to other's lists; this
        index is unchanged.  0: stored id in [a1, a2); 1: id % a1 == a2; 2: a range of every list's entries"""
        _check(_L.mvs_index_ivf_copy_subset_to(self._h, other._h, int(subset_type), int(a1), int(a2)))

    def range_search(self, x, radius, nprobe=0, efSearch=0, sel=None):
        """faiss.Index.range_search -> (lims [nq + 1] int64, D [lims[-1]] float32, I [lims[-1]] int64): query q's hits are entries
        lims[q]:lims[q + 1]; a hit has dis < radius (L2) / dis > radius (inner product), strict -- the "range search" block of include/mi355_faiss.h"""
        x = _f32(x).reshape(-1, self.d)
        nq = x.shape[0]
        p, keep = make_params(nprobe, efSearch, sel)
        r = _p()
        _check(_L.mvs_index_range_search(self._h, nq, _ptr(x), C.c_float(float(radius)), C.byref(p), C.byref(r)))
        del keep
        try:
            n = _L.mvs_range_result_nq(r)
            lims = np.ctypeslib.as_array(_L.mvs_range_result_lims(r), shape=(n + 1,)).copy()
            total = int(lims[-1])
            if total > 0:
                D = np.ctypeslib.as_array(_L.mvs_range_result_distances(r), shape=(total,)).copy()
                I = np.ctypeslib.as_array(_L.mvs_range_result_labels(r), shape=(total,)).copy()
            else:
                D, I = np.empty(0, dtype=np.float32), np.empty(0, dtype=np.int64)
        finally:
            _L.mvs_range_result_free(r)
        return lims, D, I

    # ---- reconstruct (include/mi355_faiss.h "reconstruct"): the row as the index stores it, as d float32 values
    def reconstruct(self, key):
        """faiss.Index.reconstruct -> [d] float32"""
        out = np.empty(self.d, dtype=np.float32)
        _check(_L.mvs_index_reconstruct(self._h, int(key), _ptr(out)))
        return out

    def reconstruct_n(self, i0, ni, out=None):
        """faiss.Index.reconstruct_n -> [ni, d] float32.  out: a C-contiguous float32 array of ni * d values to write into -- a bare IVF
        index leaves the rows of absent ids in it untouched"""
        ni = int(ni)
        if out is None:
            out = np.empty((max(ni, 0), self.d), dtype=np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == max(ni, 0) * self.d
        _check(_L.mvs_index_reconstruct_n(self._h, int(i0), ni, _ptr(out)))
        return out

    def reconstruct_batch(self, keys):
        """faiss.Index.reconstruct_batch -> [n, d] float32"""
        keys = _i64a(keys).reshape(-1)
        out = np.empty((keys.size, self.d), dtype=np.float32)
        _check(_L.mvs_index_reconstruct_batch(self._h, keys.size, _ptr(keys), _ptr(out)))
        return out

    def search_and_reconstruct(self, x, k, nprobe=0, efSearch=0, sel=None):
        """faiss.Index.search_and_reconstruct -> (D [nq, k], I [nq, k], R [nq, k, d]): D and I as search gives them, R[q, j] the
        reconstruction of I[q, j]; every byte 0xFF where I[q, j] is -1"""
        x = _f32(x).reshape(-1, self.d)
        nq = x.shape[0]
        D = np.empty((nq, max(k, 0)), dtype=np.float32)
        I = np.empty((nq, max(k, 0)), dtype=np.int64)
        R = np.empty((nq, max(k, 0), self.d), dtype=np.float32)
        p, keep = make_params(nprobe, efSearch, sel)
        _check(_L.mvs_index_search_and_reconstruct(self._h, nq, _ptr(x), k, _ptr(D), _ptr(I), _ptr(R), C.byref(p)))
        del keep
        return D, I, R

    def to_gpu(self, device):
        """faiss_to_gpu(name, device): src/gpu/gpu.cpp:48 (in place)"""
        _check(_L.mvs_index_to_gpu(self._h, int(device)))

    def clone_to_gpu(self, device):
        """faiss.index_cpu_to_gpu(res, device, index): returns a new index on `device`"""
        h = _p()
        _check(_L.mvs_index_clone_to_gpu(C.byref(h), self._h, int(device)))
        return Index(h)

    def prefilter_stats(self):
        q, f, e, b = _i64(0), _i64(0), C.c_float(0), C.c_float(0)
        _check(_L.mvs_index_prefilter_stats(self._h, C.byref(q), C.byref(f), C.byref(e), C.byref(b)))
        return {"queries": q.value, "fallback_queries": f.value, "max_rel_err": e.value, "err_bound": b.value}

    def ivf_probe_stats(self):
        """(query, list) pairs of the last IVF coarse-filter search and how many of them were scanned (probe pruning)."""
        a, b, c, e = _i64(0), _i64(0), _i64(0), _i64(0)
        _check(_L.mvs_index_ivf_probe_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(e)))
        return {"pairs": a.value, "scanned": b.value, "forced_drains": c.value, "admitted": e.value}

    def get_stat(self, name):
        """a named diagnostic counter -- include/mi355_faiss.h mvs_index_get_stat"""
        v = _i64(0)
        _check(_L.mvs_index_get_stat(self._h, name.encode(), C.byref(v)))
        return v.value

    def shadow_stats(self):
        """Flat L2: the shadow clustering's state, size and cost -- include/mi355_faiss.h mvs_index_shadow_stats"""
        st, sec = (_i64 * 8)(), C.c_double(0)
        _check(_L.mvs_index_shadow_stats(self._h, st, C.byref(sec)))
        keys = ("state", "rows", "queries", "unproven", "builds", "extends", "device_bytes", "nlist")
        out = {k: int(v) for k, v in zip(keys, st)}
        out["build_seconds"] = sec.value
        return out

    def collect_stats(self):
        q, c, o = _i64(0), _i64(0), _i64(0)
        _check(_L.mvs_index_collect_stats(self._h, C.byref(q), C.byref(c), C.byref(o)))
        return {"queries": q.value, "candidates": c.value, "overflows": o.value}

    def shard_to_gpus(self, devices):
        """spread this index over `devices` in place (row shards; HNSW: replicas) -- include/mi355_faiss.h"""
        arr = (C.c_int * len(devices))(*[int(v) for v in devices])
        _check(_L.mvs_index_shard_to_gpus(self._h, arr, len(devices)))

    def shard_info(self):
        """-> None (not sharded) | dict(devices, rows_per_shard, last_tie_queries)"""
        devs, rows, ties = (C.c_int * 64)(), (_i64 * 64)(), _i64(0)
        n = _L.mvs_index_shard_info(self._h, devs, 64, rows, C.byref(ties))
        if n <= 0:
            return None
        return {"devices": list(devs[:n]), "rows_per_shard": list(rows[:n]), "last_tie_queries": ties.value}

    # ---- device-resident variants (torch tensors on the index's device) ----
    def add_torch(self, x, ids=None, stream=None):
        import torch

        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(
            _L.mvs_index_add_device(
                self._h, x.shape[0], x.data_ptr(), ids.data_ptr() if ids is not None else None, stream
            )
        )

    def search_torch(self, x, k, D=None, I=None, nprobe=0, efSearch=0, sel=None, stream=None):
        import torch

        assert x.is_cuda and x.is_contiguous()
        nq = x.shape[0]
        if D is None:
            D = torch.empty((nq, k), dtype=torch.float32, device=x.device)
        if I is None:
            I = torch.empty((nq, k), dtype=torch.int64, device=x.device)
        p, keep = make_params(nprobe, efSearch, sel)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(_L.mvs_index_search_device(self._h, nq, x.data_ptr(), k, D.data_ptr(), I.data_ptr(), C.byref(p), stream))
        del keep
        return D, I

    def reconstruct_batch_torch(self, keys, out=None, stream=None):
        """keys: int64 tensor on the index's device -> [n, d] float32 tensor there (mvs_index_reconstruct_batch_device)"""
        import torch

        assert keys.is_cuda and keys.dtype == torch.int64 and keys.is_contiguous()
        n = keys.numel()
        if out is None:
            out = torch.empty((n, self.d), dtype=torch.float32, device=keys.device)
        if stream is None:
            stream = torch.cuda.current_stream(keys.device).cuda_stream
        _check(_L.mvs_index_reconstruct_batch_device(self._h, n, keys.data_ptr(), out.data_ptr(), stream))
        return out

    def search_and_reconstruct_torch(self, x, k, nprobe=0, efSearch=0, sel=None, stream=None):
        """-> (D, I, R) tensors on x's device; nothing visits the host (mvs_index_search_and_reconstruct_device)"""
        import torch

        assert x.is_cuda and x.is_contiguous()
        nq = x.shape[0]
        D = torch.empty((nq, k), dtype=torch.float32, device=x.device)
        I = torch.empty((nq, k), dtype=torch.int64, device=x.device)
        R = torch.empty((nq, k, self.d), dtype=torch.float32, device=x.device)
        p, keep = make_params(nprobe, efSearch, sel)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(_L.mvs_index_search_and_reconstruct_device(self._h, nq, x.data_ptr(), k, D.data_ptr(), I.data_ptr(), R.data_ptr(), C.byref(p), stream))
        del keep
        return D, I, R

    def ivf_tie_emit_torch(self, flagged, xq, T, k, sel=None, stream=None):
        """IVF row shard: for the flagged queries (int64 tensor of query numbers of the batch `xq` that has JUST been searched on this
        index) this shard's first k rows not worse than T in arrival order: (value f32, stored id i64, probe rank i32), each [nf, k],
        -1 padded -- include/mi355_faiss.h mvs_index_ivf_tie_emit_device"""
        import torch

        nf = int(flagged.shape[0])
        dev = xq.device
        v = torch.zeros((nf, k), dtype=torch.float32, device=dev)
        ids = torch.full((nf, k), -1, dtype=torch.int64, device=dev)
        rk = torch.full((nf, k), -1, dtype=torch.int32, device=dev)
        if nf == 0:
            return v, ids, rk
        flag = torch.empty(nf + 1, dtype=torch.int32, device=dev)
        flag[0] = nf
        flag[1:] = flagged.to(torch.int32)
        p, keep = make_params(0, 0, sel)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(_L.mvs_index_ivf_tie_emit_device(self._h, nf, C.c_void_p(flag.data_ptr()), C.c_void_p(xq.data_ptr()), C.c_void_p(T.data_ptr()),
                                                int(k), C.c_void_p(v.data_ptr()), C.c_void_p(ids.data_ptr()), C.c_void_p(rk.data_ptr()),
                                                C.byref(p), C.c_void_p(stream)))
        del keep
        return v, ids, rk

    def tie_candidates_torch(self, xf, T, k, sel=None, stream=None):
        """per flagged query the k smallest GLOBAL rows with score >= T (ascending, -1 padded) -- include/mi355_faiss.h"""
        import torch

        nf = xf.shape[0]
        out = torch.empty((nf, k), dtype=torch.int64, device=xf.device)
        p, keep = make_params(0, 0, sel)
        if stream is None:
            stream = torch.cuda.current_stream(xf.device).cuda_stream
        _check(_L.mvs_index_tie_candidates_device(self._h, nf, xf.data_ptr(), T.data_ptr(), k, out.data_ptr(), C.byref(p), stream))
        del keep
        return out

    def set_label_offset(self, off):
        _check(_L.mvs_index_set_label_offset(self._h, int(off)))

    def set_option(self, key, value):
        _check(_L.mvs_index_set_option(self._h, key.encode(), int(value)))

    def set_kernel_timing(self, on):
        _check(_L.mvs_index_set_kernel_timing(self._h, 1 if on else 0))

    def kernel_time_stats(self):
        n, t = C.c_int(0), C.c_double(0)
        _check(_L.mvs_index_kernel_time_stats(self._h, C.byref(n), C.byref(t)))
        return n.value, t.value

    def last_kernel_info(self):
        ki = KernelInfo()
        _check(_L.mvs_index_last_kernel_info(self._h, C.byref(ki)))
        return {
            "name": ki.name.decode(), "flops": ki.flops, "bytes": ki.bytes, "last_ms": ki.last_ms,
            "grid": ki.grid, "block": ki.block, "lds_bytes": ki.lds_bytes, "nsplit": ki.nsplit,
        }  # fmt: skip


BINARY_KIND_FLAT = 1
BINARY_KIND_IDMAP = 2


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


class IndexBinary:
    """Device-native binary index (faiss.IndexBinary): rows of d bits as code_size = d / 8 uint8 values, Hamming distances as int32 --
    the "binary indexes" section of include/mi355_faiss.h."""

    def __init__(self, handle, owned=True, parent=None):
        self._h = handle
        self._owned = owned
        self._parent = parent  # keeps the owning index alive for borrowed handles

    def __del__(self, _free=_L.mvs_binary_index_free, _finalizing=sys.is_finalizing):
        # (as Index.__del__: nothing is freed while the interpreter finalizes)
        if getattr(self, "_h", None) and getattr(self, "_owned", False) and not _finalizing():
            _free(self._h)
        self._h = None

    d = property(lambda s: _L.mvs_binary_index_d(s._h))
    code_size = property(lambda s: _L.mvs_binary_index_code_size(s._h))
    ntotal = property(lambda s: _L.mvs_binary_index_ntotal(s._h))
    kind = property(lambda s: _L.mvs_binary_index_kind(s._h))
    is_trained = property(lambda s: True)
    metric_type = property(lambda s: 1)

    @property
    def index(self):
        """IndexBinaryIDMap::index: the wrapped IndexBinaryFlat (labels are row numbers), None on a bare index"""
        h = _L.mvs_binary_index_idmap_sub(self._h)
        return IndexBinary(h, owned=False, parent=self) if h else None

    def train(self, x):
        pass

    def _rows(self, x):
        return _u8(x).reshape(-1, self.code_size)

    def add(self, x):
        x = self._rows(x)
        _check(_L.mvs_binary_index_add(self._h, x.shape[0], _ptr(x)))

    def add_with_ids(self, x, ids):
        x = self._rows(x)
        ids = _i64a(ids)
        assert ids.size == x.shape[0]
        _check(_L.mvs_binary_index_add_with_ids(self._h, x.shape[0], _ptr(x), _ptr(ids)))

    def search(self, x, k, sel=None):
        """-> (D [nq, k] int32, I [nq, k] int64): the k smallest (ham, row) pairs per query; padding is (2147483647, -1)"""
        x = self._rows(x)
        nq = x.shape[0]
        D = np.empty((nq, max(k, 0)), dtype=np.int32)
        I = np.empty((nq, max(k, 0)), dtype=np.int64)
        p, keep = make_params(0, 0, sel)
        _check(_L.mvs_binary_index_search(self._h, nq, _ptr(x), k, _ptr(D), _ptr(I), C.byref(p)))
        del keep
        return D, I

    def range_search(self, x, radius, sel=None):
        """-> (lims [nq + 1] int64, D [lims[-1]] float32, I [lims[-1]] int64): a hit has ham < radius, strictly; hits in row order"""
        x = self._rows(x)
        nq = x.shape[0]
        p, keep = make_params(0, 0, sel)
        r = _p()
        _check(_L.mvs_binary_index_range_search(self._h, nq, _ptr(x), int(radius), C.byref(p), C.byref(r)))
        del keep
        try:
            n = _L.mvs_range_result_nq(r)
            lims = np.ctypeslib.as_array(_L.mvs_range_result_lims(r), shape=(n + 1,)).copy()
            total = int(lims[-1])
            if total > 0:
                D = np.ctypeslib.as_array(_L.mvs_range_result_distances(r), shape=(total,)).copy()
                I = np.ctypeslib.as_array(_L.mvs_range_result_labels(r), shape=(total,)).copy()
            else:
                D, I = np.empty(0, dtype=np.float32), np.empty(0, dtype=np.int64)
        finally:
            _L.mvs_range_result_free(r)
        return lims, D, I

    def reset(self):
        _check(_L.mvs_binary_index_reset(self._h))

    def reconstruct(self, key):
        out = np.empty(self.code_size, dtype=np.uint8)
        _check(_L.mvs_binary_index_reconstruct(self._h, int(key), _ptr(out)))
        return out

    def reconstruct_n(self, i0, ni):
        ni = int(ni)
        out = np.empty((max(ni, 0), self.code_size), dtype=np.uint8)
        _check(_L.mvs_binary_index_reconstruct_n(self._h, int(i0), ni, _ptr(out)))
        return out

    # ---- device-resident variants (uint8 torch tensors on the index's device) ----
    def add_torch(self, x, ids=None, stream=None):
        import torch

        assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous()
        assert ids is None or (ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() == x.shape[0])
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(_L.mvs_binary_index_add_device(self._h, x.shape[0], x.data_ptr(), ids.data_ptr() if ids is not None else None, stream))

    def search_torch(self, x, k, D=None, I=None, sel=None, stream=None):
        import torch

        assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous()
        nq = x.shape[0]
        if D is None:
            D = torch.empty((nq, k), dtype=torch.int32, device=x.device)
        if I is None:
            I = torch.empty((nq, k), dtype=torch.int64, device=x.device)
        p, keep = make_params(0, 0, sel)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(_L.mvs_binary_index_search_device(self._h, nq, x.data_ptr(), k, D.data_ptr(), I.data_ptr(), C.byref(p), stream))
        del keep
        return D, I

    def set_option(self, key, value):
        _check(_L.mvs_binary_index_set_option(self._h, key.encode(), int(value)))

    def get_stat(self, name):
        v = _i64(0)
        _check(_L.mvs_binary_index_get_stat(self._h, name.encode(), C.byref(v)))
        return int(v.value)


def index_binary_factory(d, description):
    """faiss.index_binary_factory: "BFlat", "IDMap,BFlat", "IDMap2,BFlat"; d in bits"""
    h = _p()
    _check(_L.mvs_binary_index_factory(C.byref(h), d, description.encode()))
    return IndexBinary(h)


def write_index_binary(index, filename):
    _check(_L.mvs_write_index_binary(index._h, os.fsencode(filename)))


def read_index_binary(filename):
    h = _p()
    _check(_L.mvs_read_index_binary(C.byref(h), os.fsencode(filename)))
    return IndexBinary(h)


def index_factory(d, description, metric=METRIC_INNER_PRODUCT):
    """faiss.index_factory; default metric INNER_PRODUCT as the extension (src/faiss_extension.cpp:105)"""
    h = _p()
    _check(_L.mvs_index_factory(C.byref(h), int(d), description.encode(), int(metric)))
    return Index(h)


def write_index(index, filename):
    _check(_L.mvs_write_index(index._h, filename.encode()))


def read_index(filename):
    h = _p()
    _check(_L.mvs_read_index(C.byref(h), filename.encode()))
    return Index(h)


def merge_shards(metric, D, I):
    """Host k-way merge after the all-gather: D, I [nshard, nq, k] (global labels) -> [nq, k]"""
    D, I = _f32(D), _i64a(I)
    ns, nq, k = D.shape
    Do = np.empty((nq, k), dtype=np.float32)
    Io = np.empty((nq, k), dtype=np.int64)
    _check(_L.mvs_merge_shards(metric, nq, k, ns, _ptr(D), _ptr(I), _ptr(Do), _ptr(Io)))
    return Do, Io


def merge_records_torch(metric, rec, kout, raw=False):
    """device merge of gathered records: rec [nshard, nq, kk, 2] int64 (torch, on the GPU) -> (D [nq, kout] f32, I [nq, kout]
    i64) torch tensors on the same device; raw: pure order instead of FAISS's print order"""
    import torch

    ns, nq, kk, _ = rec.shape
    D = torch.empty((nq, kout), dtype=torch.float32, device=rec.device)
    I = torch.empty((nq, kout), dtype=torch.int64, device=rec.device)
    st = torch.cuda.current_stream(rec.device).cuda_stream
    _check(_L.mvs_merge_records_device(int(metric), nq, kk, int(kout), ns, C.c_void_p(rec.data_ptr()), 1 if raw else 0,
                                       C.c_void_p(D.data_ptr()), C.c_void_p(I.data_ptr()), C.c_void_p(st)))
    return D, I


def merge_shards_raw(metric, D, I):
    """[nshard, nq, kk] blocks -> merged top-kk per query in the PURE order (score desc / dist asc, id asc)"""
    D, I = _f32(D), _i64a(I)
    ns, nq, kk = D.shape
    Do = np.empty((nq, kk), dtype=np.float32)
    Io = np.empty((nq, kk), dtype=np.int64)
    _check(_L.mvs_merge_shards_raw(metric, nq, kk, ns, _ptr(D), _ptr(I), _ptr(Do), _ptr(Io)))
    return Do, Io


def finish_ip_ties(k, rawD, rawI, flagged, first_rows):
    """FAISS print order of the first k of every raw list + the CMin-heap outcome for the flagged queries"""
    rawD, rawI = _f32(rawD), _i64a(rawI)
    nq, kk = rawD.shape
    flagged, first_rows = _i64a(flagged), _i64a(first_rows)
    Do = np.empty((nq, k), dtype=np.float32)
    Io = np.empty((nq, k), dtype=np.int64)
    _check(_L.mvs_finish_ip_ties(nq, k, kk, _ptr(rawD), _ptr(rawI), flagged.size, _ptr(flagged), _ptr(first_rows), _ptr(Do), _ptr(Io)))
    return Do, Io


def synth_uniform_torch(n, d, seed, row0=0, device="cuda:0", out=None):
    import torch

    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=device)
    st = torch.cuda.current_stream(out.device).cuda_stream
    _check(_L.mvs_synth_uniform_device(out.data_ptr(), n, d, seed, row0, st))
    return out


def mfma_bf16_16x16x32(A_bits, Bt_bits, C):
    """D = A B + C by ONE v_mfma_f32_16x16x32_bf16 per tile (diagnostics): A_bits [n][16][32], Bt_bits [n][16][32] uint16 bf16
    patterns (Bt = the columns of B as rows), C [n][16][16] float32"""
    import numpy as np

    A_bits = np.ascontiguousarray(A_bits, dtype=np.uint16)
    Bt_bits = np.ascontiguousarray(Bt_bits, dtype=np.uint16)
    Cc = np.ascontiguousarray(C, dtype=np.float32)
    n = A_bits.shape[0]
    assert A_bits.shape == (n, 16, 32) and Bt_bits.shape == (n, 16, 32) and Cc.shape == (n, 16, 16)
    D = np.empty((n, 16, 16), dtype=np.float32)
    _check(_L.mvs_debug_mfma_bf16_16x16x32(A_bits.ctypes.data, Bt_bits.ctypes.data, Cc.ctypes.data, D.ctypes.data, n))
    return D


def synth_clustered_torch(n, d, seed, row0=0, n_centers=1024, sigma=0.1, device="cuda:0", out=None):
    import torch

    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=device)
    st = torch.cuda.current_stream(out.device).cuda_stream
    _check(_L.mvs_synth_clustered_device(out.data_ptr(), n, d, seed, row0, n_centers, sigma, st))
    return out
