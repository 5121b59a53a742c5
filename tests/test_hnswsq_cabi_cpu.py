"""CPU-side checks of the HNSW<M>,SQ8 boundary: the header defines the kind and carries the contract's key phrases, the Python host
exports the constant, and the tests' own IHNs writer and parser agree with each other."""
import os
import re

import numpy as np

import faiss_format as ff
import hnswsq_reference as hsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")
L2, IP = hsr.L2, hsr.IP


def test_header_defines_the_kind_and_carries_the_contract():
    full = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define\s+MVS_KIND_HNSWSQ\s+9\b", src)
    assert re.search(r"#define\s+MVS_KIND_HNSW\s+4\b", src) and re.search(r"#define\s+MVS_KIND_IVFSQ\s+8\b", src)
    for phrase in ("HNSW<M>,SQ8", "HNSW<M>_SQ8", "faiss::IndexHNSWSQ", "IHNs", "IxSQ", "a[k] + (float)c * s[k]", "never an fma", "vdiff / 255.0f",
                   "vmin + 0.5f * s", "(int)(255.0f * clamp((x - vmin) / vdiff, 0, 1))", "the point's own DECODED row", "RAW row as the query",
                   "hnsw_build_waves = 1", "hnsw_bf16 is ignored", "hnsw_row_bytes", "hnsw_store_bytes", "dp = ceil(d / 4) * 4",
                   "This index type is not implemented"):
        assert phrase in full, phrase
    # the block sits after the SQ8 one
    assert full.index("8-bit scalar-quantised indexes") < full.index("HNSW over 8-bit scalar-quantised rows")


def test_python_host_exports_the_kind():
    import mi355_faiss as mf

    assert mf.KIND_HNSWSQ == 9 and mf.KIND_HNSW == 4
    for method in ("sq_trained", "sq_set_trained", "sq_codes", "hnsw_graph", "hnsw_walk_stats", "set_ef_construction"):
        assert callable(getattr(mf.Index, method)), method


def test_ihns_image_round_trips_through_the_python_writer_and_parser():
    rng = np.random.default_rng(9)
    d, M, n = 6, 4, 30
    vmin, vdiff = rng.standard_normal(d).astype(np.float32), rng.uniform(0.5, 2, d).astype(np.float32)
    codes = rng.integers(0, 256, size=(n, d), dtype=np.uint8)
    levels = np.ones(n, dtype=np.int32)
    levels[7] = 2
    offsets = np.concatenate([[0], np.cumsum((levels + 1) * M)]).astype(np.int64)
    neighbors = rng.integers(-1, n, size=int(offsets[-1])).astype(np.int32)
    g = hsr.full_graph(M, dict(levels=levels, offsets=offsets, neighbors=neighbors, entry_point=7, max_level=1), efc=55, efs=33)
    for ids in (None, rng.permutation(1000)[:n].astype(np.int64)):
        buf = hsr.write_hnswsq(None, d, IP, g, vmin, vdiff, codes, ids=ids)
        assert buf[:4] == (b"IHNs" if ids is None else b"IxMp")
        img = hsr.parse_hnswsq(buf)
        assert (img["d"], img["ntotal"], img["trained"], img["metric"]) == (d, n, True, IP)
        st, gr = img["storage"], img["graph"]
        assert (st["qtype"], st["rangestat"], st["rangestat_arg"], st["sq_code_size"]) == (0, 0, 0.0, d)
        assert np.array_equal(st["vmin"].view(np.uint32), vmin.view(np.uint32)) and np.array_equal(st["vdiff"].view(np.uint32), vdiff.view(np.uint32))
        assert np.array_equal(st["codes"], codes)
        assert np.array_equal(gr["levels"], levels) and np.array_equal(gr["offsets"].astype(np.int64), offsets) and np.array_equal(gr["neighbors"], neighbors)
        assert (gr["entry_point"], gr["max_level"], gr["efConstruction"], gr["efSearch"], gr["upper_beam"]) == (7, 1, 55, 33, 1)
        probas, cum = ff.hnsw_level_tables(M)
        assert np.array_equal(gr["assign_probas"], probas) and np.array_equal(gr["cum_nneighbor_per_level"], cum)
        assert (img["ids"] is None) if ids is None else np.array_equal(img["ids"], ids)
    # up to the storage the bytes are what the IHNf writer gives for the same graph, fourcc apart
    flat = ff.dumps({"kind": "hnswflat", "metric": IP, "graph": g, "storage": {"kind": "flat", "metric": IP, "x": np.zeros((n, d), dtype=np.float32)}})
    bare = hsr.write_hnswsq(None, d, IP, g, vmin, vdiff, codes)
    cut = bare.index(b"IxSQ")
    assert flat[:4] == b"IHNf" and flat[4:cut] == bare[4:cut] and flat[cut : cut + 4] == b"IxFI"
