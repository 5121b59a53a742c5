"""CPU model of the "<base>,RFlat" index (include/mi355_faiss.h "exact f32 re-ranking over the quantised indexes") and an independent writer /
parser of the IxRF file layout, built on the base kinds' models (pq_reference, ivfpq_reference, sq_reference) and the unchanged oracle.
A helper module: nothing here is collected.

The base's model is asked for kb ROW NUMBERS (its stored ids are the rows of the refine store), the exact values are the oracle's
pair-path chains (sq_reference.chains) and the selection is a lexsort by (value, row)."""
import struct

import numpy as np

import ivfpq_reference as ivr
import pq_reference as pqr
import sq_reference as sqr
from oracle import oracle as orc

FLT_MAX = np.finfo(np.float32).max
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
MAX_KB = 2048
BASES = ("PQ", "IVFPQ", "SQ", "IVFSQ")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def candidates(k, k_factor):
    """kb = (int64)((float)k * k_factor): an f32 product, truncated"""
    return int(np.float32(k) * np.float32(k_factor))


def refine(metric, rows, xq, cand, k, labels=None, label_offset=0, exact=None):
    """cand [nq, kb]: store rows, -1 = none -> the k best by (exact value, row), padded with -1 / +-FLT_MAX.
    exact: the chains [nq, n] if the caller has them already"""
    xq = _f32(xq)
    nq = xq.shape[0]
    l2 = metric == L2
    if exact is None:
        exact = sqr.chains(metric, rows, xq)
    D = np.full((nq, k), FLT_MAX if l2 else -FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        c = np.asarray(cand[q], dtype=np.int64)
        c = c[c >= 0]
        v = exact[q, c]
        order = np.lexsort((c, v if l2 else -v))[:k]
        D[q, : order.size] = v[order]
        I[q, : order.size] = c[order] + label_offset if labels is None else np.asarray(labels)[c[order]]
    return D, I


class Model:
    """One "<base>,RFlat" index: the base's parameters (shared with the device index through the accessors), the rows in arrival order.

    base "PQ": cb; "IVFPQ": cent, cb; "SQ": vmin, vdiff; "IVFSQ": cent, vmin, vdiff"""

    def __init__(self, base, metric, d, cent=None, cb=None, vmin=None, vdiff=None):
        assert base in BASES
        self.base, self.metric, self.d = base, metric, d
        self.cent, self.cb, self.vmin, self.vdiff = cent, cb, vmin, vdiff
        self.rows = np.empty((0, d), dtype=np.float32)
        self._built = None

    def add(self, x):
        self.rows = np.concatenate([self.rows, _f32(x).reshape(-1, self.d)])
        self._built = None

    def built(self):
        """the base's stored form of the rows: codes [n, M | d], or per list (stored ids = rows, codes)"""
        if self._built is None:
            if self.base == "PQ":
                self._built = pqr.encode(self.cb, self.rows) if len(self.rows) else np.empty((0, self.cb.shape[0]), dtype=np.uint8)
            elif self.base == "SQ":
                self._built = sqr.encode(self.vmin, self.vdiff, self.rows)
            elif self.base == "IVFPQ":
                self._built = ivr.build_lists(self.metric, self.cent, self.cb, self.rows)
            else:
                self._built = sqr.build_lists(self.metric, self.cent, self.vmin, self.vdiff, self.rows)
        return self._built

    def base_search(self, xq, kb, nprobe=1, keep=None):
        """-> rows [nq, kb] (-1 padded) in the base's own pure order; keep: bool mask over the rows (the selector's verdict)"""
        xq = _f32(xq)
        b = self.built()
        if self.base == "PQ":
            return pqr.search(self.cb, b, xq, kb, self.metric, keep=keep)[1]
        if self.base == "SQ":
            return sqr.sq_search(self.metric, self.vmin, self.vdiff, b, xq, kb, keep=keep)[1]
        keep_ids = None if keep is None else np.nonzero(np.asarray(keep, dtype=bool))[0]
        if self.base == "IVFPQ":
            return ivr.search(self.metric, self.cent, self.cb, b, xq, kb, nprobe, keep_ids=keep_ids)[1]
        return sqr.ivf_search(self.metric, self.cent, self.vmin, self.vdiff, b, xq, kb, nprobe, keep_ids=keep_ids)[1]

    def search(self, xq, k, k_factor=1.0, nprobe=1, id_map=None, keep=None, label_offset=0, exact=None):
        kb = candidates(k, k_factor)
        assert 1 <= kb <= MAX_KB
        cand = self.base_search(xq, kb, nprobe, keep)
        return refine(self.metric, self.rows, xq, cand, k, labels=id_map, label_offset=label_offset, exact=exact)

    def base_image(self, nprobe=1):
        """the base's file image (the base kinds' own writers), bare"""
        b, n = self.built(), len(self.rows)
        if self.base == "PQ":
            return pqr.write_pq(None, self.d, self.metric, self.cb, b)
        if self.base == "SQ":
            return sqr.write_sq(None, self.d, self.metric, self.vmin, self.vdiff, b)
        if self.base == "IVFPQ":
            return ivr.write_ivfpq(None, self.d, self.metric, self.cent, self.cb, b, nprobe=nprobe)
        return sqr.write_ivfsq(None, self.d, self.metric, self.cent, self.vmin, self.vdiff, b, nprobe=nprobe)

    def image(self, k_factor=1.0, id_map=None, path=None, **kw):
        return write_refine(path, self.d, self.metric, self.base_image(), self.rows, k_factor, id_map=id_map, **kw)


# ---- the IxRF file (FAISS impl/index_write.cpp IndexRefine, restated from memory): "IxRF", the index header, the base index, the refine
# index (IxF2 / IxFI: header, size_t count of floats, the rows), float k_factor; under IDMap the usual IxMp wrapper around it
def _header(d, ntotal, trained, metric):
    return struct.pack("<iqqqBi", d, ntotal, 1 << 20, 1 << 20, 1 if trained else 0, metric)


def flat_image(d, metric, rows, ntotal=None, fourcc=None):
    rows = np.ascontiguousarray(rows, dtype="<f4").reshape(-1)
    n = rows.size // d if ntotal is None else ntotal
    cc = fourcc or (b"IxF2" if metric == L2 else b"IxFI")
    return cc + _header(d, n, True, metric) + struct.pack("<Q", rows.size) + rows.tobytes()


def write_refine(path_or_none, d, metric, base_image, rows, k_factor, trained=True, id_map=None, store_image=None, ntotal=None):
    """base_image: bytes of the base index's bare image; store_image: bytes in place of the Flat image of `rows` (malformed files)"""
    n = len(rows) if ntotal is None else ntotal
    body = b"IxRF" + _header(d, n, trained, metric) + base_image + (flat_image(d, metric, rows) if store_image is None else store_image)
    body += struct.pack("<f", k_factor)
    if id_map is not None:
        id_map = np.ascontiguousarray(id_map, dtype="<i8")
        body = b"IxMp" + _header(d, n, trained, metric) + body + struct.pack("<Q", id_map.size) + id_map.tobytes()
    if path_or_none is not None:
        with open(path_or_none, "wb") as f:
            f.write(body)
    return body


_BASE_PARSERS = {b"IxPq": ("PQ", pqr.parse_pq), b"IwPQ": ("IVFPQ", ivr.parse_ivfpq), b"IxSQ": ("SQ", sqr.parse_sq), b"IwSq": ("IVFSQ", sqr.parse_ivfsq)}


def parse_refine(buf):
    """-> dict(d, ntotal, trained, metric, base_kind, base (the base parser's dict), rows [n, d], k_factor, id_map | None).  The store's
    image and the tail have a known size, so the base's image is what lies between: it goes to the base kind's own parser whole"""
    if not isinstance(buf, (bytes, bytearray)):
        buf = open(buf, "rb").read()
    hs = len(_header(1, 0, True, 0))
    pos, id_map = 0, None
    wrapped = buf[:4] == b"IxMp"
    end = len(buf)
    if wrapped:
        _, n_outer, _, _, _, _ = struct.unpack_from("<iqqqBi", buf, 4)
        pos = 4 + hs
        end -= 8 * n_outer
        id_map = np.frombuffer(buf, dtype="<i8", count=n_outer, offset=end).copy()
        end -= 8
        assert struct.unpack_from("<Q", buf, end)[0] == n_outer
    assert buf[pos : pos + 4] == b"IxRF", buf[pos : pos + 4]
    d, ntotal, _, _, trained, metric = struct.unpack_from("<iqqqBi", buf, pos + 4)
    pos += 4 + hs
    end -= 4
    (k_factor,) = struct.unpack_from("<f", buf, end)
    store_len = 4 + hs + 8 + 4 * ntotal * d
    s0 = end - store_len
    assert buf[s0 : s0 + 4] == (b"IxF2" if metric == L2 else b"IxFI"), buf[s0 : s0 + 4]
    sd, sn, _, _, strained, smetric = struct.unpack_from("<iqqqBi", buf, s0 + 4)
    assert (sd, sn, smetric, bool(strained)) == (d, ntotal, metric, True)
    (nf,) = struct.unpack_from("<Q", buf, s0 + 4 + hs)
    assert nf == ntotal * d
    rows = np.frombuffer(buf, dtype="<f4", count=nf, offset=s0 + 4 + hs + 8).reshape(ntotal, d).copy()
    base_buf = bytes(buf[pos:s0])
    kind, parser = _BASE_PARSERS[base_buf[:4]]
    return dict(d=d, ntotal=ntotal, trained=bool(trained), metric=metric, base_kind=kind, base=parser(base_buf), rows=rows, k_factor=k_factor,
                id_map=id_map)
