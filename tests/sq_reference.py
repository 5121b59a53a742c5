"""CPU model of the SQ8 and IVF<n>,SQ8 indexes (include/mi355_faiss.h "8-bit scalar-quantised indexes"), built on the unchanged oracle,
and independent writers / parsers of the IxSQ and IwSq file layouts.  A helper module: nothing here is collected.

Train, encode and decode are plain numpy f32 with one array operation per contract operation, so every one is rounded on its own; the
chains are the oracle's pair-path chains on the decoded rows."""
import struct

import numpy as np

from admission_rule import admitted
from oracle import oracle as orc

FLT_MAX = np.finfo(np.float32).max
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
F255, FHALF = np.float32(255.0), np.float32(0.5)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- the quantiser
def train_range(y):
    """y [n, d]: the rows (SQ8) or the residuals (IVF) -> (vmin [d], vdiff [d])"""
    y = _f32(y)
    vmin, vmax = y.min(axis=0), y.max(axis=0)
    return vmin, (vmax - vmin).astype(np.float32)


def derived(vmin, vdiff):
    """-> (a [d], s [d]): s = vdiff / 255, a = vmin + 0.5 s"""
    s = (_f32(vdiff) / F255).astype(np.float32)
    half = (FHALF * s).astype(np.float32)
    return (_f32(vmin) + half).astype(np.float32), s


def encode(vmin, vdiff, y):
    """-> codes [n, d] uint8: 0 where vdiff == 0, else (int)(255 clamp((y - vmin) / vdiff, 0, 1))"""
    y, vmin, vdiff = _f32(y), _f32(vmin), _f32(vdiff)
    num = (y - vmin).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        xi = (num / vdiff).astype(np.float32)
    xi = np.minimum(np.maximum(xi, np.float32(0.0)), np.float32(1.0))
    scaled = (F255 * xi).astype(np.float32)
    codes = np.where(vdiff == 0, np.float32(0.0), scaled)
    return codes.astype(np.int32).astype(np.uint8)  # (truncation)


def decode(vmin, vdiff, codes):
    """dec(c, k) = a[k] + (float)c s[k]: one multiplication, one addition -> [n, d] f32"""
    a, s = derived(vmin, vdiff)
    prod = (np.asarray(codes).astype(np.float32) * s).astype(np.float32)
    return (a + prod).astype(np.float32)


def chains(metric, rows, xq):
    """[nq, n]: the pair-path chain (L2: fmaf(t, t, acc), t = x - y; inner product: fmaf(x, y, acc)) of every query against every row,
    evaluated directly (oracle pair_chains), so a query may hold NaN, inf or values whose squares overflow"""
    return orc.pair_chains(metric, _f32(rows), _f32(xq))


def chains_by_search(metric, rows, xq):
    """the same values read off the oracle's k = n search: finite input only (the search applies the heap's admission rule).
    tests/test_admission_rule_cpu.py holds chains() to it bit for bit"""
    rows, xq = _f32(rows), _f32(xq)
    n = rows.shape[0]
    out = np.empty((xq.shape[0], n), dtype=np.float32)
    if n == 0:
        return out
    D, I = orc.flat_search_naive(metric, rows, xq, n, orc.PATH_PAIR)
    assert (np.sort(I, axis=1) == np.arange(n)).all()
    out[np.arange(xq.shape[0])[:, None], I] = D
    return out


# ---- SQ8
def sq_distances(metric, vmin, vdiff, codes, xq):
    return chains(metric, decode(vmin, vdiff, codes), xq)


def sq_select(dis, k, metric, labels=None, keep=None):
    """dis [nq, n] -> of the values the heap rule admits (tests/admission_rule.py) the k best per query in the pure order (distance, then
    internal row), padded with -1 / +-FLT_MAX; labels: id_map; keep: bool mask over rows (selector)"""
    nq, n = dis.shape
    l2 = metric == L2
    D = np.full((nq, k), FLT_MAX if l2 else -FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    rows_all = np.arange(n)
    if keep is not None:
        rows_all = rows_all[np.asarray(keep, dtype=bool)]
    for q in range(nq):
        rows = rows_all[admitted(metric, dis[q, rows_all])]
        dq = dis[q, rows]
        order = np.lexsort((rows, dq if l2 else -dq))[:k]
        D[q, : order.size] = dq[order]
        I[q, : order.size] = rows[order] if labels is None else np.asarray(labels)[rows[order]]
    return D, I


def sq_search(metric, vmin, vdiff, codes, xq, k, labels=None, keep=None):
    return sq_select(sq_distances(metric, vmin, vdiff, codes, xq), k, metric, labels, keep)


# ---- IVF<n>,SQ8
def assign(metric, cent, x):
    """-> (list of every row [n], per list the row numbers in list order): what IVF<n>,Flat with these centroids does on add"""
    cent, x = _f32(cent), _f32(x)
    nlist, d = cent.shape
    ix = orc.Index(d, f"IVF{nlist},Flat", metric)
    ix.ivf_set_centroids(cent)
    if x.shape[0]:
        ix.add_with_ids(x, np.arange(x.shape[0], dtype=np.int64))
    of_row = np.full(x.shape[0], -1, dtype=np.int64)
    rows = []
    for l in range(nlist):
        r, _ = ix.ivf_list(l)
        of_row[r] = l
        rows.append(r)
    return of_row, rows


def residuals(cent, x, of_row):
    """r[k] = x[k] - c[k], one f32 subtraction per component"""
    return (_f32(x) - _f32(cent)[of_row]).astype(np.float32)


def ivf_train(x, nlist, metric):
    """-> (coarse centroids [nlist, d], vmin [d], vdiff [d]); the range over the residuals"""
    x = _f32(x)
    ix = orc.Index(x.shape[1], f"IVF{nlist},Flat", metric)
    ix.train(x)
    cent = ix.ivf_centroids()
    of_row, _ = assign(metric, cent, x)
    assert (of_row >= 0).all()
    return (cent,) + train_range(residuals(cent, x, of_row))


def build_lists(metric, cent, vmin, vdiff, x, ids=None):
    """-> per list (stored ids [n_l] int64, codes [n_l, d] uint8) in list order; ids default to the sequence numbers"""
    x = _f32(x)
    d = x.shape[1]
    ids = np.arange(x.shape[0], dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    if x.shape[0] == 0:
        return [(np.empty(0, dtype=np.int64), np.empty((0, d), dtype=np.uint8)) for _ in range(cent.shape[0])]
    of_row, rows = assign(metric, cent, x)
    assert (of_row >= 0).all()
    codes = encode(vmin, vdiff, residuals(cent, x, of_row))
    return [(ids[r], codes[r]) for r in rows]


def probes(metric, cent, xq, nprobe):
    """the probed lists of every query in rank order [nq, min(nprobe, nlist)]"""
    _, P = orc.flat_search(metric, _f32(cent), _f32(xq), min(nprobe, cent.shape[0]))
    return P


def pair_distances(metric, cent_l, vmin, vdiff, xq, codes):
    """dis [nq, n_l] of the queries against one list's codes"""
    xq = _f32(xq)
    dec = decode(vmin, vdiff, codes)
    if metric == L2:
        return chains(L2, dec, (xq - cent_l).astype(np.float32))
    base = chains(IP, _f32(cent_l[None]), xq)  # [nq, 1]: the chain <x, c>
    return (base + chains(IP, dec, xq)).astype(np.float32)


def all_pair_distances(metric, cent, vmin, vdiff, lists, xq):
    """per list dis [nq, n_l] of EVERY query against it (None for an empty list): a pair's value does not depend on its probe rank"""
    return [pair_distances(metric, cent[l], vmin, vdiff, xq, codes_l) if ids_l.size else None for l, (ids_l, codes_l) in enumerate(lists)]


def ivf_select(metric, P, lists, dis_lists, k, id_map=None, keep_ids=None):
    """P [nq, np]: the probed lists in rank order (-1: none) -> of the values the heap rule admits the k best per query in the pure order (distance, probe rank, position in
    the list), padded with -1 / +-FLT_MAX.  id_map: stored id -> label (IDMap); keep_ids: the labels a selector admits"""
    nq = P.shape[0]
    D = np.full((nq, k), FLT_MAX if metric == L2 else -FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    labels, kept = [], []
    for ids_l, _ in lists:
        lab = ids_l if id_map is None else np.asarray(id_map)[ids_l]
        labels.append(lab)
        kept.append(np.arange(lab.size) if keep_ids is None else np.nonzero(np.isin(lab, keep_ids))[0])
    for q in range(nq):
        parts = [(dis_lists[l][q, kept[l]], np.full(kept[l].size, r), kept[l], labels[l][kept[l]]) for r, l in enumerate(P[q]) if l >= 0 and kept[l].size]
        if not parts:
            continue
        dis, rank, pos, lab = (np.concatenate(c) for c in zip(*parts))
        adm = admitted(metric, dis)  # the heap rule (tests/admission_rule.py), then the pure order among what it admits
        dis, rank, pos, lab = dis[adm], rank[adm], pos[adm], lab[adm]
        key = dis if metric == L2 else -dis
        if key.size > k:  # only entries not worse than the k-th value can be among the k best
            m = key <= np.partition(key, k - 1)[k - 1]
            key, dis, rank, pos, lab = key[m], dis[m], rank[m], pos[m], lab[m]
        order = np.lexsort((pos, rank, key))[:k]
        D[q, : order.size] = dis[order]
        I[q, : order.size] = lab[order]
    return D, I


def ivf_search(metric, cent, vmin, vdiff, lists, xq, k, nprobe, id_map=None, keep_ids=None):
    xq = _f32(xq)
    return ivf_select(metric, probes(metric, cent, xq, nprobe), lists, all_pair_distances(metric, cent, vmin, vdiff, lists, xq), k, id_map, keep_ids)


# ---- the files (FAISS impl/index_write.cpp, restated).  ScalarQuantizer block: int qtype, int rangestat, float rangestat_arg, size_t d,
# size_t code_size, vector<float> trained (vmin [d] | vdiff [d]).  IxSQ: header, block, vector<uint8> codes.  IwSq: the ivf header as IwFl
# writes it (header, size_t nlist, nprobe, the quantizer index, direct map), block, size_t code_size, uint8 by_residual, the lists
def _header(d, ntotal, trained, metric):
    return struct.pack("<iqqqBi", d, ntotal, 1 << 20, 1 << 20, 1 if trained else 0, metric)


def _sq_block(d, vmin, vdiff, qtype=0, code_size=None):
    tr = np.concatenate([_f32(vmin).reshape(-1), _f32(vdiff).reshape(-1)]).astype("<f4")
    return struct.pack("<iifQQ", qtype, 0, 0.0, d, d if code_size is None else code_size) + struct.pack("<Q", tr.size) + tr.tobytes()


def _wrap(body, d, ntotal, trained, metric, id_map, path):
    if id_map is not None:
        id_map = np.ascontiguousarray(id_map, dtype="<i8")
        body = b"IxMp" + _header(d, ntotal, trained, metric) + body + struct.pack("<Q", id_map.size) + id_map.tobytes()
    if path is not None:
        with open(path, "wb") as f:
            f.write(body)
    return body


def write_sq(path_or_none, d, metric, vmin, vdiff, codes, trained=True, ids=None, qtype=0):
    codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1, d)
    n = codes.shape[0]
    body = b"IxSQ" + _header(d, n, trained, metric) + _sq_block(d, vmin, vdiff, qtype) + struct.pack("<Q", codes.size) + codes.tobytes()
    return _wrap(body, d, n, trained, metric, ids, path_or_none)


def write_ivfsq(path_or_none, d, metric, cent, vmin, vdiff, lists, nprobe=1, trained=True, id_map=None, by_residual=1, qtype=0, code_size=None):
    """cent None: an index whose quantizer is still empty"""
    nlist = len(lists)
    ntotal = sum(int(i.size) for i, _ in lists)
    cs = d if code_size is None else code_size
    body = b"IwSq" + _header(d, ntotal, trained, metric) + struct.pack("<QQ", nlist, nprobe)
    rows = np.empty(0, dtype="<f4") if cent is None else np.ascontiguousarray(cent, dtype="<f4").reshape(-1)
    body += (b"IxF2" if metric == L2 else b"IxFI") + _header(d, rows.size // d, True, metric) + struct.pack("<Q", rows.size) + rows.tobytes()
    body += struct.pack("<bQ", 0, 0)  # DirectMap::NoMap, empty array
    body += _sq_block(d, vmin, vdiff, qtype, cs) + struct.pack("<QB", cs, by_residual)
    body += b"ilar" + struct.pack("<QQ", nlist, cs)
    sizes = [int(i.size) for i, _ in lists]
    if sum(1 for s in sizes if s) > nlist // 2:
        body += b"full" + struct.pack("<Q", nlist) + struct.pack(f"<{nlist}Q", *sizes)
    else:
        flat = [v for l, s in enumerate(sizes) if s for v in (l, s)]
        body += b"sprs" + struct.pack("<Q", len(flat)) + struct.pack(f"<{len(flat)}Q", *flat)
    for ids_l, codes_l in lists:
        if ids_l.size:
            body += np.ascontiguousarray(codes_l, dtype=np.uint8).reshape(-1, d).tobytes() + np.ascontiguousarray(ids_l, dtype="<i8").tobytes()
    return _wrap(body, d, ntotal, trained, metric, id_map, path_or_none)


class _Cursor:
    def __init__(self, buf):
        self.buf = buf if isinstance(buf, (bytes, bytearray)) else open(buf, "rb").read()
        self.pos = 0

    def take(self, fmt):
        v = struct.unpack_from(fmt, self.buf, self.pos)
        self.pos += struct.calcsize(fmt)
        return v

    def array(self, dtype, count):
        a = np.frombuffer(self.buf, dtype=dtype, count=count, offset=self.pos).copy()
        self.pos += a.nbytes
        return a

    def header(self):
        d, ntotal, _, _, trained, metric = self.take("<iqqqBi")
        assert metric <= 1
        return d, ntotal, bool(trained), metric

    def fourcc(self):
        return bytes(self.take("<4s")[0])

    def sq_block(self, d):
        qtype, rangestat, rangestat_arg, d2, code_size = self.take("<iifQQ")
        assert d2 == d
        (nt,) = self.take("<Q")
        tr = self.array("<f4", nt)
        assert nt in (0, 2 * d)
        return dict(qtype=qtype, rangestat=rangestat, rangestat_arg=rangestat_arg, sq_code_size=code_size,
                    vmin=tr[:d] if nt else None, vdiff=tr[d:] if nt else None)

    def finish(self, wrapped):
        id_map = None
        if wrapped:
            (nid,) = self.take("<Q")
            id_map = self.array("<i8", nid)
        assert self.pos == len(self.buf), (self.pos, len(self.buf))
        return id_map


def parse_sq(buf):
    """-> dict(d, ntotal, trained, metric, qtype, rangestat, rangestat_arg, sq_code_size, vmin, vdiff, codes [n, d], ids | None)"""
    c = _Cursor(buf)
    cc = c.fourcc()
    wrapped = cc == b"IxMp"
    if wrapped:
        c.header()
        cc = c.fourcc()
    assert cc == b"IxSQ", cc
    d, ntotal, trained, metric = c.header()
    out = dict(d=d, ntotal=ntotal, trained=trained, metric=metric, **c.sq_block(d))
    (nc,) = c.take("<Q")
    out["codes"] = c.array(np.uint8, nc).reshape(-1, d)
    out["ids"] = c.finish(wrapped)
    return out


def parse_ivfsq(buf):
    """-> dict(d, ntotal, trained, metric, nlist, nprobe, centroids [nlist or 0, d], the block's fields, code_size, by_residual,
    lists [(ids, codes)], id_map | None)"""
    c = _Cursor(buf)
    cc = c.fourcc()
    wrapped = cc == b"IxMp"
    if wrapped:
        c.header()
        cc = c.fourcc()
    assert cc == b"IwSq", cc
    d, ntotal, trained, metric = c.header()
    nlist, nprobe = c.take("<QQ")
    qcc = c.fourcc()
    assert qcc in (b"IxF2", b"IxFI", b"IxFl"), qcc
    qd, qn, _, _ = c.header()
    assert qd == d
    (nf,) = c.take("<Q")
    assert nf == qn * d
    cent = c.array("<f4", nf).reshape(-1, d)
    dm_type, dm_n = c.take("<bQ")
    assert dm_type == 0 and dm_n == 0
    out = dict(d=d, ntotal=ntotal, trained=trained, metric=metric, nlist=nlist, nprobe=nprobe, centroids=cent, **c.sq_block(d))
    code_size, by_residual = c.take("<QB")
    assert c.fourcc() == b"ilar"
    nl2, cs2 = c.take("<QQ")
    assert nl2 == nlist and cs2 == code_size
    kind = c.fourcc()
    (ns,) = c.take("<Q")
    raw = c.array("<u8", ns)
    sizes = np.zeros(nlist, dtype=np.int64)
    if kind == b"full":
        assert ns == nlist
        sizes[:] = raw
    else:
        assert kind == b"sprs", kind
        sizes[raw[0::2].astype(np.int64)] = raw[1::2]
    lists = []
    for l in range(nlist):
        codes = c.array(np.uint8, int(sizes[l]) * code_size).reshape(-1, code_size)
        lists.append((c.array("<i8", int(sizes[l])), codes))
    out.update(code_size=code_size, by_residual=by_residual, lists=lists, id_map=c.finish(wrapped))
    return out
