"""CPU model of the binary indexes (include/mi355_faiss.h "binary indexes"), numpy only.

Rows and queries are uint8 arrays of code_size = d / 8 bytes.  Everything the device returns is compared with this model bit for bit:
distances are integers, so there is no tolerance anywhere."""
import struct

import numpy as np

PAD_DISTANCE = 2147483647
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


def ham(xq, xb):
    """[nq, n] int32: popcount of q XOR r over the code bytes, by a 256-entry table"""
    xq = np.ascontiguousarray(xq, dtype=np.uint8)
    xb = np.ascontiguousarray(xb, dtype=np.uint8)
    out = np.zeros((xq.shape[0], xb.shape[0]), dtype=np.int32)
    for j in range(xq.shape[1]):
        out += POPCOUNT[xq[:, j, None] ^ xb[None, :, j]]
    return out


def member(sel, ids):
    """membership of the ids in a selector ("bitmap", uint8 bytes) | ("batch", int64 ids), by the rules of the remove_ids section:
    a negative id and an id beyond the bitmap are no members; duplicates in a batch are harmless"""
    ids = np.asarray(ids, dtype=np.int64)
    if sel is None:
        return np.ones(ids.shape, dtype=bool)
    kind, data = sel
    if kind == "bitmap":
        bits = np.ascontiguousarray(data, dtype=np.uint8)
        ok = (ids >= 0) & ((ids >> 3) < bits.size)
        safe = np.where(ok, ids, 0)
        return ok & (((bits[safe >> 3] if bits.size else np.zeros(ids.shape, np.uint8)) >> (safe & 7).astype(np.uint8)) & 1).astype(bool)
    if kind == "batch":
        return np.isin(ids, np.asarray(data, dtype=np.int64))
    raise ValueError(kind)


def _labels(n, id_map):
    return np.arange(n, dtype=np.int64) if id_map is None else np.asarray(id_map, dtype=np.int64)


def search(xb, xq, k, sel=None, id_map=None, dist=None):
    """the k smallest (ham, row) pairs of the admitted rows per query; missing slots are (2147483647, -1).
    dist: a precomputed ham(xq, xb) to share between tests"""
    n, nq = len(xb), len(xq)
    lab = _labels(n, id_map)
    rows = np.nonzero(member(sel, lab))[0]
    D = np.full((nq, k), PAD_DISTANCE, dtype=np.int32)
    I = np.full((nq, k), -1, dtype=np.int64)
    if n == 0 or rows.size == 0:
        return D, I
    dis = ham(xq, xb) if dist is None else dist
    for q in range(nq):
        h = dis[q, rows]
        order = np.lexsort((rows, h))[:k]
        D[q, : order.size] = h[order]
        I[q, : order.size] = lab[rows[order]]
    return D, I


def range_search(xb, xq, radius, sel=None, id_map=None, dist=None):
    """(lims, D float32, I): row r is a hit iff ham < radius, strictly; a query's hits in ascending row order"""
    n, nq = len(xb), len(xq)
    lab = _labels(n, id_map)
    lims = np.zeros(nq + 1, dtype=np.int64)
    Ds, Is = [], []
    if n:
        ok = member(sel, lab)
        dis = ham(xq, xb) if dist is None else dist
        for q in range(nq):
            rows = np.nonzero(ok & (dis[q] < radius))[0]
            lims[q + 1] = lims[q] + rows.size
            Ds.append(dis[q, rows].astype(np.float32))
            Is.append(lab[rows])
    D = np.concatenate(Ds) if Ds else np.empty(0, np.float32)
    I = np.concatenate(Is) if Is else np.empty(0, np.int64)
    return lims, D, I


def same_range(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


# ---- the two file formats, written and parsed independently of the library


def _header(cc, d, ntotal):
    return cc + struct.pack("<iiqBi", d, d // 8, ntotal, 1, 1)


def write_image(xb, d, id_map=None, idmap2=False, code_size=None, nbytes=None):
    """the bytes of an "IBxF" file, or of "IBMp" / "IBM2" around it.  code_size / nbytes: wrong values on purpose"""
    xb = np.ascontiguousarray(xb, dtype=np.uint8).reshape(-1, d // 8)
    n = xb.shape[0]
    flat = _header(b"IBxF", d, n)
    if code_size is not None:
        flat = b"IBxF" + struct.pack("<iiqBi", d, code_size, n, 1, 1)
    flat += struct.pack("<Q", xb.size if nbytes is None else nbytes) + xb.tobytes()
    if id_map is None:
        return flat
    ids = np.ascontiguousarray(id_map, dtype=np.int64)
    return _header(b"IBM2" if idmap2 else b"IBMp", d, n) + flat + struct.pack("<Q", ids.size) + ids.tobytes()


class ParseError(ValueError):
    pass


def parse_image(buf):
    """-> dict(kind "IBxF" | "IBMp" | "IBM2", d, ntotal, codes [ntotal, d / 8] uint8, ids int64 or None); ParseError on a bad file"""
    pos = 0

    def take(n, what):
        nonlocal pos
        if pos + n > len(buf):
            raise ParseError("truncated at %s: %d bytes wanted at offset %d of %d" % (what, n, pos, len(buf)))
        out = buf[pos : pos + n]
        pos += n
        return out

    def header():
        d, cs, ntotal, trained, metric = struct.unpack("<iiqBi", take(21, "header"))
        if d <= 0 or d % 8:
            raise ParseError("d = %d" % d)
        if cs != d // 8:
            raise ParseError("code_size = %d for d = %d" % (cs, d))
        if ntotal < 0:
            raise ParseError("ntotal = %d" % ntotal)
        return d, ntotal

    def flat_body(d, ntotal):
        (nb,) = struct.unpack("<Q", take(8, "codes size"))
        if nb != ntotal * (d // 8):
            raise ParseError("codes hold %d bytes, ntotal x code_size = %d" % (nb, ntotal * (d // 8)))
        return np.frombuffer(take(nb, "codes"), dtype=np.uint8).reshape(ntotal, d // 8).copy()

    cc = bytes(take(4, "fourcc"))
    if cc == b"IBxF":
        d, ntotal = header()
        out = dict(kind="IBxF", d=d, ntotal=ntotal, codes=flat_body(d, ntotal), ids=None)
    elif cc in (b"IBMp", b"IBM2"):
        d, ntotal = header()
        if bytes(take(4, "sub fourcc")) != b"IBxF":
            raise ParseError("sub-index is not IBxF")
        d2, n2 = header()
        if (d2, n2) != (d, ntotal):
            raise ParseError("sub-index header disagrees")
        codes = flat_body(d, ntotal)
        (ni,) = struct.unpack("<Q", take(8, "id_map size"))
        if ni != ntotal:
            raise ParseError("id_map holds %d ids, ntotal = %d" % (ni, ntotal))
        ids = np.frombuffer(take(8 * ni, "id_map"), dtype=np.int64).copy()
        out = dict(kind=cc.decode(), d=d, ntotal=ntotal, codes=codes, ids=ids)
    else:
        raise ParseError("fourcc %r is not a binary index" % cc)
    if pos != len(buf):
        raise ParseError("%d bytes after the image" % (len(buf) - pos))
    return out
