"""CPU model of the HNSW<M>,SQ8 index (include/mi355_faiss.h "HNSW over 8-bit scalar-quantised rows"), built on the unchanged oracle and on
tests/sq_reference.py, and an independent writer / parser of the IHNs file layout.  A helper module: nothing here is collected.

The index is HNSW<M> over the DECODED rows y_i = dec(enc(x_i)): train / encode / decode are sq_reference's (one numpy f32 operation per
contract operation), the graph and the walk are the oracle's HNSW<M> fed the rows y and searched with the caller's raw queries."""
import struct

import numpy as np

import faiss_format as ff
import sq_reference as sqr
from oracle import oracle as orc

L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT


class Model:
    """range + codes + the oracle's HNSW<M> over the decoded rows"""

    def __init__(self, d, M, metric, train_rows, idmap=False, efc=None, vmin=None, vdiff=None):
        self.d, self.M, self.metric, self.idmap = d, M, metric, idmap
        if vmin is None:
            vmin, vdiff = sqr.train_range(train_rows)
        self.vmin, self.vdiff = sqr._f32(vmin), sqr._f32(vdiff)
        self.codes = np.empty((0, d), dtype=np.uint8)
        self.index = orc.Index(d, ("IDMap," if idmap else "") + f"HNSW{M}", metric)
        if efc:
            self.index.hnsw_set_ef_construction(efc)

    def add(self, x, ids=None):
        codes = sqr.encode(self.vmin, self.vdiff, x)
        y = sqr.decode(self.vmin, self.vdiff, codes)
        self.codes = np.concatenate([self.codes, codes])
        if self.idmap:
            self.index.add_with_ids(y, ids)
        else:
            self.index.add(y)

    def decoded(self):
        return sqr.decode(self.vmin, self.vdiff, self.codes)

    def graph(self):
        return self.index.hnsw_graph()

    def search(self, xq, k, **kw):
        return self.index.search(xq, k, **kw)


def codes_are_distinct(codes):
    """exact distance ties are where the oracle's two pop-min rules part: a parity test runs on pairwise distinct code rows only"""
    return np.unique(codes, axis=0).shape[0] == codes.shape[0]


# ---- the file.  IHNs: the common header and the HNSW block exactly as IHNf has them (tests/faiss_format.py), then the storage as an IxSQ image
# (tests/sq_reference.py: header, ScalarQuantizer block with qtype 0, vector<uint8> codes)
def _hnsw_block(w, g):
    w.vec(g["assign_probas"], np.float64)
    w.vec(g["cum_nneighbor_per_level"], np.int32)
    w.vec(g["levels"], np.int32)
    w.vec(g["offsets"], np.uint64)
    w.vec(g["neighbors"], np.int32)
    w.pack("iiiii", g["entry_point"], g["max_level"], g["efConstruction"], g["efSearch"], 1)


def full_graph(M, g, efc=40, efs=16):
    """the oracle's / the device's hnsw_graph() dict -> the dict of the file's HNSW block"""
    probas, cum = ff.hnsw_level_tables(M)
    return dict(assign_probas=probas, cum_nneighbor_per_level=cum, levels=g["levels"], offsets=g["offsets"], neighbors=g["neighbors"],
                entry_point=g["entry_point"], max_level=g["max_level"], efConstruction=efc, efSearch=efs)


def write_hnswsq(path_or_none, d, metric, graph, vmin, vdiff, codes, trained=True, ids=None, fourcc="IHNs", flat_rows=None):
    """graph: full_graph(...).  fourcc / flat_rows build the two mismatched files: IHNf over an IxSQ storage, IHNs over a Flat one"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1, d)
    n = codes.shape[0]
    w = ff._W()
    w.cc(fourcc)
    ff._header(w, d, n, trained, metric)
    _hnsw_block(w, graph)
    if flat_rows is None:
        storage = sqr.write_sq(None, d, metric, vmin, vdiff, codes, trained=trained)
    else:
        storage = ff.dumps({"kind": "flat", "metric": metric, "x": flat_rows})
    body = w.b.getvalue() + storage
    return sqr._wrap(body, d, n, trained, metric, ids, path_or_none)


def parse_hnswsq(buf):
    """-> dict(d, ntotal, trained, metric, graph {...}, storage {parse_sq's dict}, ids | None); asserts on anything outside the layout"""
    buf = buf if isinstance(buf, (bytes, bytearray)) else open(buf, "rb").read()
    r = ff._R(buf)
    cc = r.cc()
    wrapped = cc == "IxMp"
    if wrapped:
        ff._read_header(r)
        cc = r.cc()
    assert cc == "IHNs", cc
    h = ff._read_header(r)
    g = {
        "assign_probas": r.vec(np.float64),
        "cum_nneighbor_per_level": r.vec(np.int32),
        "levels": r.vec(np.int32),
        "offsets": r.vec(np.uint64),
        "neighbors": r.vec(np.int32),
    }
    g["entry_point"], g["max_level"], g["efConstruction"], g["efSearch"], g["upper_beam"] = r.unpack("iiiii")
    # the storage: an IxSQ image that ends where the file (or the id_map) begins
    tail = 0
    if wrapped:
        (nid,) = struct.unpack_from("<Q", buf, len(buf) - 8 * (h["ntotal"] + 1))
        assert nid == h["ntotal"], (nid, h["ntotal"])
        tail = 8 * (h["ntotal"] + 1)
    st = sqr.parse_sq(bytes(buf[r.o : len(buf) - tail]))
    assert st["d"] == h["d"] and st["ntotal"] == h["ntotal"] and st["metric"] == h["metric"]
    ids = np.frombuffer(buf, dtype="<i8", count=h["ntotal"], offset=len(buf) - 8 * h["ntotal"]).copy() if wrapped else None
    return dict(d=h["d"], ntotal=h["ntotal"], trained=h["is_trained"], metric=h["metric"], graph=g, storage=st, ids=ids)
