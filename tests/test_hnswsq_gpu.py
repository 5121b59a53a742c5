"""HNSW<M>,SQ8 on the device against the CPU model of tests/hnswsq_reference.py: the oracle's HNSW<M> over the decoded rows.  With one
build wave (option hnsw_build_waves = 1) codes, graph, labels and distances are compared BITWISE (distances as uint32); with the default
concurrent build only recall is comparable.  Exact distance ties are where the oracle's two pop-min rules part, so every parity test first
asserts that its own code rows are pairwise distinct."""
import os
import subprocess
import sys

import numpy as np
import pytest

import faiss_format as ff
import hnswsq_reference as hsr
import sq_reference as sqr
from helpers import bitmap_from_ids
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "duckdb-faiss-ext_amd", "host", "boundary_driver")
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
FMAX = np.finfo(np.float32).max


def _mf():
    import mi355_faiss as mf

    return mf


def _same(D, I, Dr, Ir, what):
    assert np.array_equal(I, Ir), f"{what}: labels differ in {(I != Ir).sum()} slots, first query {np.argwhere(I != Ir)[0][0]}"
    assert np.array_equal(D.view(np.uint32), Dr.view(np.uint32)), f"{what}: distances differ in {(D != Dr).sum()} slots"


def _same_graph(a, b):
    assert a["max_level"] == b["max_level"] and a["entry_point"] == b["entry_point"]
    assert np.array_equal(a["levels"], b["levels"]) and np.array_equal(a["offsets"], b["offsets"])
    if not np.array_equal(a["neighbors"], b["neighbors"]):
        bad = np.flatnonzero(a["neighbors"] != b["neighbors"])
        v = int(np.searchsorted(a["offsets"], bad[0], side="right") - 1)
        raise AssertionError(f"{len(bad)} neighbour slots differ; first at vertex {v}: "
                             f"{a['neighbors'][a['offsets'][v]:a['offsets'][v+1]]} vs {b['neighbors'][b['offsets'][v]:b['offsets'][v+1]]}")


def _pair(d, M, metric, xb, idmap=False, ids=None, efc=None, chunk=None, waves=1, desc=None):
    """-> (model, device index), both trained on xb and holding it"""
    mf = _mf()
    m = hsr.Model(d, M, metric, xb, idmap=idmap, efc=efc)
    g = mf.index_factory(d, desc or (("IDMap," if idmap else "") + f"HNSW{M},SQ8"), metric)
    g.set_option("hnsw_build_waves", waves)
    assert not g.is_trained
    g.train(xb)
    assert g.is_trained
    if efc:
        g.set_ef_construction(efc)
    step = chunk or len(xb)
    for i in range(0, len(xb), step):
        if idmap:
            m.add(xb[i : i + step], ids[i : i + step])
            g.add_with_ids(xb[i : i + step], ids[i : i + step])
        else:
            m.add(xb[i : i + step])
            g.add(xb[i : i + step])
    assert hsr.codes_are_distinct(m.codes), "the parity tests need pairwise distinct code rows"
    return m, g


def _rows(kind, n, d, seed):
    return orc.synth_uniform(n, d, seed) if kind == "uniform" else orc.synth_clustered(n, d, seed, n_centers=16, sigma=0.5)


# ------------------------------------------------------------------------------------------------ graph and codes: the edges of the lane layout
SHAPES = [
    (7, 4, 600, "uniform"),       # a padded last word
    (100, 8, 1500, "uniform"),    # 25 of 64 lanes busy
    (260, 16, 1200, "uniform"),   # NI = 2, second step nearly empty
    (768, 32, 1200, "clustered"),  # NI = 3
    (1536, 16, 700, "clustered"),  # NI = 6
    (2048, 8, 400, "clustered"),   # NI = 8, the limit
]


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d,M,n,kind", SHAPES)
def test_codes_and_graph_equal_the_model(metric, d, M, n, kind):
    mf = _mf()
    xb = _rows(kind, n, d, 21 if kind == "uniform" else 40)
    m, g = _pair(d, M, metric, xb)
    assert g.kind == mf.KIND_HNSWSQ and g.ntotal == n
    vmin, vdiff = g.sq_trained()
    assert np.array_equal(vmin.view(np.uint32), m.vmin.view(np.uint32)) and np.array_equal(vdiff.view(np.uint32), m.vdiff.view(np.uint32))
    assert np.array_equal(g.sq_codes(), m.codes)
    _same_graph(m.graph(), g.hnsw_graph())
    assert g.get_stat("hnsw_row_bytes") == (d + 3) // 4 * 4
    xq = _rows(kind, 16, d, 22 if kind == "uniform" else 41)
    _same(*g.search(xq, 10, efSearch=64), *m.search(xq, 10, efSearch=64), f"d = {d}")


# ------------------------------------------------------------------------------------------------ search
@pytest.fixture(scope="module")
def searched():
    d, n = 64, 6000
    out = {}
    for metric in (L2, IP):
        xb = orc.synth_uniform(n, d, 24)
        out[metric] = _pair(d, 16, metric, xb)
    return out, orc.synth_uniform(333, d, 25)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("efs,k", [(16, 10), (8, 40), (300, 100), (64, 1)])
def test_search_bit_exact_on_the_same_graph(searched, metric, efs, k):
    pairs, xq = searched
    m, g = pairs[metric]
    _same_graph(m.graph(), g.hnsw_graph())
    _same(*g.search(xq, k, efSearch=efs), *m.search(xq, k, efSearch=efs), f"efSearch = {efs}, k = {k}")


def test_lists_in_lds_and_in_registers_agree(searched):
    """option hnsw_reg_lists = 0 keeps the candidate / result lists in LDS; hnsw_bf16 is ignored for this kind"""
    pairs, xq = searched
    m, g = pairs[L2]
    ref = m.search(xq, 10, efSearch=128)
    try:
        g.set_option("hnsw_reg_lists", 0)
        _same(*g.search(xq, 10, efSearch=128), *ref, "LDS lists")
        g.set_option("hnsw_bf16", 0)
        _same(*g.search(xq, 10, efSearch=128), *ref, "hnsw_bf16 = 0")
    finally:
        g.set_option("hnsw_reg_lists", 1)
        g.set_option("hnsw_bf16", 1)
    _same(*g.search(xq, 10, efSearch=128), *ref, "register lists")


def test_constant_column_decodes_to_vmin():
    d, n = 20, 1500
    xb = orc.synth_uniform(n, d, 51)
    xb[:, 5] = np.float32(0.375)
    m, g = _pair(d, 8, L2, xb)
    assert m.vdiff[5] == 0 and np.all(m.codes[:, 5] == 0) and np.all(m.decoded()[:, 5] == np.float32(0.375))
    assert np.array_equal(g.sq_codes(), m.codes)
    _same_graph(m.graph(), g.hnsw_graph())
    xq = orc.synth_uniform(40, d, 52)
    _same(*g.search(xq, 10, efSearch=32), *m.search(xq, 10, efSearch=32), "constant column")


def test_incremental_adds_like_duckdb_chunks():
    xb = orc.synth_clustered(5000, 48, 22, n_centers=32, sigma=0.2)
    m, g = _pair(48, 16, L2, xb, chunk=2048)
    assert np.array_equal(g.sq_codes(), m.codes)
    _same_graph(m.graph(), g.hnsw_graph())


def test_ef_construction_is_honoured_directly_and_through_idmap():
    d, n = 24, 2000
    xb = orc.synth_uniform(n, d, 23)
    m, g = _pair(d, 8, L2, xb, efc=100)
    _same_graph(m.graph(), g.hnsw_graph())
    m40 = hsr.Model(d, 8, L2, xb)
    m40.add(xb)
    assert not np.array_equal(m40.graph()["neighbors"], m.graph()["neighbors"])
    ids = np.arange(n, dtype=np.int64) * 5 + 3
    mi, gi = _pair(d, 8, L2, xb, idmap=True, ids=ids, efc=100)
    _same_graph(m.graph(), gi.hnsw_graph())


def test_selectors_under_idmap():
    d, n = 32, 5000
    xb, xq = orc.synth_uniform(n, d, 28), orc.synth_uniform(64, d, 29)
    ids = (np.arange(n, dtype=np.int64) * 3 + 100)[::-1].copy()
    m, g = _pair(d, 16, IP, xb, idmap=True, ids=ids, efc=64)
    keep = ids[(np.arange(n) % 4) == 0]
    bm = bitmap_from_ids(ids, (np.arange(n) % 4) == 0)
    for sel in (None, ("batch", keep), ("bitmap", bm)):
        Dg, Ig = g.search(xq, 10, efSearch=48, sel=sel)
        _same(Dg, Ig, *m.search(xq, 10, efSearch=48, sel=sel), sel and sel[0])
        if sel:
            assert np.all(np.isin(Ig[Ig >= 0], keep))


def test_edge_cases():
    mf = _mf()
    d = 8
    xb, xq = orc.synth_uniform(50, d, 31), orc.synth_uniform(5, d, 30)
    g = mf.index_factory(d, "HNSW8,SQ8", IP)
    g.set_option("hnsw_build_waves", 1)
    D, I = g.search(xq, 3)
    assert np.all(I == -1) and np.all(D == -FMAX)  # empty (and untrained) index
    g.train(xb)
    D, I = g.search(xq, 3)
    assert np.all(I == -1) and np.all(D == -FMAX)  # empty index
    with pytest.raises(mf.FaissException, match="add_with_ids not implemented for this type of index"):
        g.add_with_ids(xq, np.arange(5))
    with pytest.raises(mf.FaissException, match="k > 0"):
        g.search(xq, 0)
    m = hsr.Model(d, 8, IP, xb)
    g.add(xb[:1])  # a single vertex: entry point, no links
    m.add(xb[:1])
    D, I = g.search(xq, 3)
    assert np.all(I[:, 0] == 0) and np.all(I[:, 1:] == -1)
    _same(D, I, *m.search(xq, 3), "single vertex")
    g.add(xb[1:])
    m.add(xb[1:])
    assert hsr.codes_are_distinct(m.codes)
    _same_graph(m.graph(), g.hnsw_graph())
    _same(*g.search(xq, 64, efSearch=4), *m.search(xq, 64, efSearch=4), "k > ntotal, k > efSearch")


# ------------------------------------------------------------------------------------------------ files, placement
@pytest.mark.parametrize("idmap", [False, True])
def test_files_clone_and_refused_sharding(idmap, tmp_path):
    mf = _mf()
    d, M, n = 21, 8, 1500
    xb, xq = orc.synth_uniform(n, d, 61), orc.synth_uniform(20, d, 62)
    ids = (np.arange(n, dtype=np.int64) * 7 + 11)[::-1].copy() if idmap else None
    m, g = _pair(d, M, IP, xb, idmap=idmap, ids=ids)
    ref = m.search(xq, 10, efSearch=40)
    _same(*g.search(xq, 10, efSearch=40), *ref, "device")
    # write_index -> the Python parser reads the model's range, codes and graph
    path = str(tmp_path / "a.index")
    mf.write_index(g, path)
    img = hsr.parse_hnswsq(path)
    st, gr, mg = img["storage"], img["graph"], m.graph()
    assert (img["d"], img["ntotal"], img["trained"], img["metric"]) == (d, n, True, IP)
    assert (st["qtype"], st["rangestat"], st["rangestat_arg"], st["sq_code_size"], st["trained"]) == (0, 0, 0.0, d, True)
    assert np.array_equal(st["vmin"].view(np.uint32), m.vmin.view(np.uint32)) and np.array_equal(st["vdiff"].view(np.uint32), m.vdiff.view(np.uint32))
    assert np.array_equal(st["codes"], m.codes)
    probas, cum = ff.hnsw_level_tables(M)
    # (the probabilities come from two exp implementations: compared as tests/test_index_io_gpu.py compares them, to 1e-12 relative)
    assert np.allclose(gr["assign_probas"], probas, rtol=1e-12) and np.array_equal(gr["cum_nneighbor_per_level"], cum)
    assert np.array_equal(gr["levels"], mg["levels"]) and np.array_equal(gr["offsets"].astype(np.int64), mg["offsets"])
    assert np.array_equal(gr["neighbors"], mg["neighbors"])
    assert (gr["entry_point"], gr["max_level"], gr["efConstruction"], gr["upper_beam"]) == (mg["entry_point"], mg["max_level"], 40, 1)
    assert (img["ids"] is None) if ids is None else np.array_equal(img["ids"], ids)
    # read_index of it, and of a Python-written file, search identically
    back = mf.read_index(path)
    inner = back.index if idmap else back
    assert inner.kind == mf.KIND_HNSWSQ and back.ntotal == n and back.is_trained and np.array_equal(back.sq_codes(), m.codes)
    _same(*back.search(xq, 10, efSearch=40), *ref, "after read_index")
    path2 = str(tmp_path / "b.index")
    hsr.write_hnswsq(path2, d, IP, hsr.full_graph(M, mg), m.vmin, m.vdiff, m.codes, ids=ids)
    py = mf.read_index(path2)
    _same_graph(mg, py.hnsw_graph())
    _same(*py.search(xq, 10, efSearch=40), *ref, "from a Python-written file")
    # the two mismatched fourcc / storage combinations are refused
    path3, path4 = str(tmp_path / "c.index"), str(tmp_path / "d.index")
    hsr.write_hnswsq(path3, d, IP, hsr.full_graph(M, mg), m.vmin, m.vdiff, m.codes, ids=ids, flat_rows=m.decoded())
    with pytest.raises(mf.FaissException, match="IHNs"):
        mf.read_index(path3)
    hsr.write_hnswsq(path4, d, IP, hsr.full_graph(M, mg), m.vmin, m.vdiff, m.codes, ids=ids, fourcc="IHNf")
    with pytest.raises(mf.FaissException, match="IHNf"):
        mf.read_index(path4)
    # clone_to_gpu(0): independent of later adds; to_gpu(0) in place
    clone = g.clone_to_gpu(0)
    g.add(xq) if ids is None else g.add_with_ids(xq, np.arange(20) + 10**6)
    assert clone.ntotal == n and g.ntotal == n + 20
    _same(*clone.search(xq, 10, efSearch=40), *ref, "clone")
    clone.to_gpu(0)
    _same(*clone.search(xq, 10, efSearch=40), *ref, "clone after to_gpu")
    # sharding is refused and leaves the index intact
    with pytest.raises(mf.FaissException, match="This index type is not implemented"):
        clone.shard_to_gpus([0, 0])
    with pytest.raises(mf.FaissException, match="This index type is not implemented"):
        clone.clone_to_gpu(-1)
    assert clone.shard_info() is None and clone.ntotal == n
    _same(*clone.search(xq, 10, efSearch=40), *ref, "after the refused sharding")
    # an untrained, empty index round-trips too
    path5 = str(tmp_path / "e.index")
    mf.write_index(mf.index_factory(d, ("IDMap," if idmap else "") + "HNSW8,SQ8", L2), path5)
    empty = mf.read_index(path5)
    assert not empty.is_trained and empty.ntotal == 0 and empty.d == d


def test_sharded_factory_is_refused():
    """env MVS_DEVICES at creation: a fresh process, as the variable is read when the index is made"""
    code = (
        "import sys; sys.path.insert(0, %r); import mi355_faiss as mf\n"
        "try:\n    mf.index_factory(8, 'IDMap,HNSW8,SQ8', 1)\nexcept mf.FaissException as e:\n    print('REFUSED', e)\n"
    ) % os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, MVS_DEVICES="0,0"))
    assert out.returncode == 0, out.stderr
    assert "REFUSED" in out.stdout and "This index type is not implemented" in out.stdout


# ------------------------------------------------------------------------------------------------ factory, errors
def test_factory_strings_refusals_and_errors():
    mf = _mf()
    for desc, M in (("HNSW16,SQ8", 16), ("HNSW16_SQ8", 16), ("HNSW,SQ8", 32), ("IDMap,HNSW4,SQ8", 4), ("IDMap2,HNSW4_SQ8", 4)):
        ix = mf.index_factory(12, desc, IP)
        inner = ix.index if desc.startswith("IDMap") else ix
        assert inner.kind == mf.KIND_HNSWSQ and not ix.is_trained and ix.ntotal == 0
    assert mf.index_factory(2048, "HNSW8,SQ8", L2).d == 2048
    for desc, dd in (("HNSW16,SQ4", 8), ("HNSW16,PQ4", 8), ("HNSW16,SQfp16", 8), ("HNSW16_2L", 8), ("HNSW16,SQ8", 2049), ("IDMap,HNSW16,SQ6", 8)):
        with pytest.raises(mf.FaissException, match="This index type is not implemented on the MI355X path yet: .*" + desc.split(",", 1)[-1][-3:]):
            mf.index_factory(dd, desc, L2)
    with pytest.raises(mf.FaissException, match="metric type 2 is not implemented on the MI355X path"):
        mf.index_factory(8, "HNSW8,SQ8", 2)
    # HNSW<M> and HNSW<M>,Flat keep their kind and need no training
    for desc in ("HNSW8", "HNSW8,Flat"):
        f = mf.index_factory(8, desc, L2)
        assert f.kind == mf.KIND_HNSW and f.is_trained
        with pytest.raises(mf.FaissException, match="not an SQ index"):
            f.sq_trained()
        with pytest.raises(mf.FaissException, match="not an SQ8 index"):
            f.sq_codes()
    x = orc.synth_uniform(60, 8, 71)
    ix = mf.index_factory(8, "HNSW8,SQ8", L2)
    with pytest.raises(mf.FaissException, match="'is_trained'"):
        ix.add(x)
    with pytest.raises(mf.FaissException, match="n > 0"):
        ix.train(x[:0])
    assert not ix.is_trained and ix.ntotal == 0
    ix.train(x[:30])
    ix.train(x)  # again, while empty
    vmin, vdiff = sqr.train_range(x)
    assert np.array_equal(ix.sq_trained()[0], vmin) and np.array_equal(ix.sq_trained()[1], vdiff)
    ix.add(x)
    with pytest.raises(mf.FaissException, match="training again is only possible while it is empty"):
        ix.train(x)
    with pytest.raises(mf.FaissException, match="training again is only possible while it is empty"):
        ix.sq_set_trained(vmin, vdiff)
    # sq_set_trained marks an empty index trained
    jx = mf.index_factory(8, "IDMap,HNSW8,SQ8", L2)
    jx.sq_set_trained(vmin, vdiff)
    assert jx.is_trained
    jx.add_with_ids(x, np.arange(60, dtype=np.int64) + 9)
    assert np.array_equal(jx.sq_codes(), sqr.encode(vmin, vdiff, x))


# ------------------------------------------------------------------------------------------------ stats
def test_row_and_store_bytes():
    """the SQ8 store is 4x (6x with the bf16 copy of the first look) smaller by construction; the factor 3 leaves room for the growth policies"""
    mf = _mf()
    d, n = 100, 3000
    xb, xq = orc.synth_uniform(n, d, 81), orc.synth_uniform(8, d, 82)
    f = mf.index_factory(d, "HNSW8", L2)
    s = mf.index_factory(d, "HNSW8,SQ8", L2)
    s.train(xb)
    for ix in (f, s):
        ix.add(xb)
        ix.set_kernel_timing(True)
        ix.search(xq, 5, efSearch=32)
    assert s.get_stat("hnsw_row_bytes") == 100 and f.get_stat("hnsw_row_bytes") == 400
    assert s.get_stat("hnsw_store_bytes") >= n * 100
    assert 3 * s.get_stat("hnsw_store_bytes") < f.get_stat("hnsw_store_bytes")
    ws = s.hnsw_walk_stats()
    assert ws["evaluations"] > 0 and ws["f32_rows"] == ws["evaluations"] and ws["bf16_rows"] == 0


# ------------------------------------------------------------------------------------------------ the glue
def test_idmap_hnsw_sq8_through_the_cpp_glue_path():
    """boundary_driver ingest: chunked AddFunction from two threads (buffered: the index needs training), AddFinaliseFunction (train + add)"""
    out = subprocess.run([DRIVER, "ingest", "3000", "8", "2", "IDMap,HNSW8,SQ8"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ingest\tOK ntotal=3000" in out.stdout


# ------------------------------------------------------------------------------------------------ the default concurrent build
def test_concurrent_build_recall():
    """default build = many waves under per-vertex locks: the graph differs from the single-thread order, recall must not (margin 0.02, as
    tests/test_hnsw_gpu.py test_concurrent_build_recall)"""
    mf = _mf()
    d, n = 64, 20000
    xb = orc.synth_clustered(n, d, 32, n_centers=256, sigma=0.25)
    xq = orc.synth_clustered(300, d, 33, n_centers=256, sigma=0.25)
    g = mf.index_factory(d, "HNSW32,SQ8", L2)
    g.train(xb)
    for i in range(0, n, 2048):
        g.add(xb[i : i + 2048])
    gr = g.hnsw_graph()
    nb, off = gr["neighbors"], gr["offsets"]
    for v in range(0, n, 97):  # structural invariants survive the concurrency
        lst = nb[off[v] : off[v] + 64]
        used = lst[lst >= 0]
        assert np.all(lst[: len(used)] >= 0) and np.all(lst[len(used) :] == -1)
        assert len(set(used.tolist())) == len(used) and v not in used
        assert np.all((used >= 0) & (used < n))
    m = hsr.Model(d, 32, L2, xb)
    m.add(xb)
    assert np.array_equal(g.sq_codes(), m.codes)
    _, If = orc.flat_search(L2, xb, xq, 10)

    def recall(I):
        return np.mean([len(set(a) & set(b)) / len(b) for a, b in zip(I, If)])

    r_dev, r_model = recall(g.search(xq, 10, efSearch=128)[1]), recall(m.search(xq, 10, efSearch=128)[1])
    print(f"recall@10 against exact Flat: device (concurrent build) {r_dev:.4f}, model {r_model:.4f}")
    assert r_dev >= r_model - 0.02, (r_dev, r_model)
