"""CPU model of reconstruct / reconstruct_n / reconstruct_batch / search_and_reconstruct (include/mi355_faiss.h "reconstruct") for every index
kind, computed from an index IMAGE -- the bytes write_index produces -- by the independent parsers of tests/faiss_format.py, sq_reference.py,
pq_reference.py, ivfpq_reference.py, hnswsq_reference.py and refine_reference.py.  A helper module: nothing here is collected.

A reconstruction is the row as the index stores it: the f32 row (Flat, HNSW, IVF,Flat, the refine store), the codebook entries of the codes
(PQ), sq_reference.decode (SQ8), and for the coded IVF kinds (decoded residual + centroid).astype(float32), one numpy f32 addition.  A key that
several rows carry names the row added LAST.  An image keeps the arrival order of a kind without lists and of the id map, but of an IVF kind only
inside each list: load(..., of_row=) takes the list of every row in arrival order (sq_reference.assign) where duplicates may sit in
different lists."""
import struct

import numpy as np

import faiss_format as ff
import hnswsq_reference as hsr
import ivfpq_reference as ivr
import pq_reference as pqr
import refine_reference as rfr
import sq_reference as sqr

_HEADER = struct.calcsize("<iqqqBi")


class KeyNotFound(KeyError):
    pass


class OutOfRange(IndexError):
    pass


def pq_decode(cb, codes):
    """cb [M, 256, dsub], codes [n, M] -> [n, M * dsub]: sub-vector m is cb[m, codes[:, m]], a copy"""
    cb = np.ascontiguousarray(cb, dtype=np.float32)
    codes = np.asarray(codes).reshape(-1, cb.shape[0])
    return np.concatenate([cb[m][codes[:, m].astype(np.int64)] for m in range(cb.shape[0])], axis=1).astype(np.float32).reshape(codes.shape[0], -1)


def add_centroid(res, cent_l):
    """the decoded residual first, then ONE f32 addition of the centroid per component"""
    return (np.ascontiguousarray(res, dtype=np.float32) + np.ascontiguousarray(cent_l, dtype=np.float32)).astype(np.float32)


class Model:
    """rows [n, d] f32: the reconstructions in image order; stored [n] | None: the stored id of each (IVF kinds; None: the position is the
    key); rank [n]: arrival rank among rows of equal stored id; id_map [m] | None: external ids by row / by stored id (IDMap)"""

    def __init__(self, d, rows, stored=None, id_map=None, lists_of=None):
        self.d = d
        self.rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, d)
        self.stored = None if stored is None else np.ascontiguousarray(stored, dtype=np.int64)
        self.rank = np.arange(self.rows.shape[0])
        self.id_map = None if id_map is None else np.ascontiguousarray(id_map, dtype=np.int64)
        self.lists_of = lists_of  # [n] the list of each image entry (IVF kinds)

    @property
    def ntotal(self):
        return self.rows.shape[0]

    @property
    def bare_ivf(self):
        return self.stored is not None and self.id_map is None

    def set_arrival(self, of_row):
        """of_row [n]: the list of every row in ARRIVAL order -> the image's entries get their arrival ranks (a list keeps arrival order)"""
        of_row = np.asarray(of_row)
        assert self.lists_of is not None and of_row.size == self.ntotal
        for l in np.unique(self.lists_of):
            mine, arrived = np.nonzero(self.lists_of == l)[0], np.nonzero(of_row == l)[0]
            assert mine.size == arrived.size, (l, mine.size, arrived.size)
            self.rank[mine] = arrived

    def _entry(self, key):
        key = int(key)
        if self.id_map is not None:
            hit = np.nonzero(self.id_map == key)[0]
            if hit.size == 0:
                raise KeyNotFound(key)
            key = int(hit[-1])  # the row of the id map added last
        if self.stored is None:
            if key < 0 or key >= self.ntotal:
                raise OutOfRange(key) if self.id_map is None else KeyNotFound(key)
            return key
        hit = np.nonzero(self.stored == key)[0]
        if hit.size == 0:
            raise KeyNotFound(key)
        return int(hit[np.argmax(self.rank[hit])])

    def reconstruct(self, key):
        return self.rows[self._entry(key)].copy()

    def reconstruct_batch(self, keys):
        """raises for the FIRST missing key in batch order"""
        keys = np.asarray(keys, dtype=np.int64).reshape(-1)
        out = np.empty((keys.size, self.d), dtype=np.float32)
        for i, k in enumerate(keys):
            out[i] = self.rows[self._entry(k)]
        return out

    def reconstruct_n(self, i0, ni, out=None):
        """a bare IVF kind writes the rows whose stored id lies in the range at id - i0 and leaves the others of `out` untouched"""
        out = np.empty((ni, self.d), dtype=np.float32) if out is None else out
        if ni == 0:
            return out
        if self.stored is None and self.id_map is None and (i0 < 0 or i0 + ni > self.ntotal):
            raise OutOfRange((i0, ni))
        for j in range(ni):
            try:
                out[j] = self.rows[self._entry(i0 + j)]
            except KeyNotFound:
                if not self.bare_ivf:
                    raise
        return out

    def of_labels(self, I):
        """[..., d]: the reconstruction of every label; every byte 0xFF where the label is -1"""
        I = np.asarray(I, dtype=np.int64)
        out = np.empty(I.shape + (self.d,), dtype=np.float32)
        flat, oi = out.reshape(-1, self.d), I.reshape(-1)
        for j, lab in enumerate(oi):
            if lab == -1:
                flat[j].view(np.uint32)[:] = 0xFFFFFFFF
            else:
                flat[j] = self.rows[self._entry(lab)]
        return out


def _from_lists(d, lists, decode, id_map):
    """lists [(ids, payload)] of an inverted-lists image -> Model; decode(l, payload) -> [size, d]"""
    rows, stored, lof = [], [], []
    for l, (ids_l, payload) in enumerate(lists):
        if len(ids_l):
            rows.append(decode(l, payload))
            stored.append(np.asarray(ids_l, dtype=np.int64))
            lof.append(np.full(len(ids_l), l))
    if not rows:
        return Model(d, np.empty((0, d), dtype=np.float32), np.empty(0, dtype=np.int64), id_map, np.empty(0, dtype=np.int64))
    return Model(d, np.concatenate(rows), np.concatenate(stored), id_map, np.concatenate(lof))


def _sq_rows(p):
    return sqr.decode(p["vmin"], p["vdiff"], p["codes"]) if p["ntotal"] else np.empty((0, p["d"]), dtype=np.float32)


def _ivfsq(p, id_map):
    return _from_lists(p["d"], p["lists"], lambda l, c: add_centroid(sqr.decode(p["vmin"], p["vdiff"], c), p["centroids"][l]), id_map)


def _ivfpq(p, id_map):
    return _from_lists(p["d"], p["lists"], lambda l, c: add_centroid(pq_decode(p["codebooks"], c), p["centroids"][l]), id_map)


def _ff(ix, id_map=None):
    kind = ix["kind"]
    if kind == "idmap":
        return _ff(ix["sub"], ix["ids"])
    if kind == "flat":
        return Model(ix["d"], ix["x"], None, id_map)
    if kind == "hnswflat":
        return Model(ix["d"], ix["storage"]["x"], None, id_map)
    assert kind == "ivfflat", kind
    return _from_lists(ix["d"], ix["lists"], lambda l, c: c, id_map)


def load(buf, of_row=None):
    """bytes or path of an index image -> Model"""
    buf = buf if isinstance(buf, (bytes, bytearray)) else open(buf, "rb").read()
    cc = bytes(buf[:4])
    if cc in (b"IxMp", b"IxM2"):
        cc = bytes(buf[4 + _HEADER : 8 + _HEADER])
    if cc == b"IxPq":
        p = pqr.parse_pq(buf)
        m = Model(p["d"], pq_decode(p["centroids"], p["codes"]) if p["ntotal"] else np.empty((0, p["d"]), dtype=np.float32), None, p["ids"])
    elif cc == b"IxSQ":
        p = sqr.parse_sq(buf)
        m = Model(p["d"], _sq_rows(p), None, p["ids"])
    elif cc == b"IwPQ":
        p = ivr.parse_ivfpq(buf)
        m = _ivfpq(p, p["id_map"])
    elif cc == b"IwSq":
        p = sqr.parse_ivfsq(buf)
        m = _ivfsq(p, p["id_map"])
    elif cc == b"IHNs":
        p = hsr.parse_hnswsq(buf)
        m = Model(p["d"], _sq_rows(p["storage"]), None, p["ids"])
    elif cc == b"IxRF":
        p = rfr.parse_refine(buf)
        m = Model(p["d"], p["rows"], None, p["id_map"])
    else:
        m = _ff(ff.loads(bytes(buf)))
    if of_row is not None:
        m.set_arrival(of_row)
    return m
