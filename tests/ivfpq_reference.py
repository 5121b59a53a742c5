"""CPU model of the IVF<n>,PQ<M> index (include/mi355_faiss.h "inverted lists of product-quantised residuals"), built on
tests/pq_reference.py and the unchanged oracle, and an independent writer / parser of the IwPQ file layout.  A helper module:
nothing here is collected."""
import struct

import numpy as np

import pq_reference as pqr
from admission_rule import admitted
from oracle import oracle as orc

FLT_MAX = pqr.FLT_MAX
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT


def assign(metric, cent, x):
    """-> (list of every row [n], per list the row numbers in list order): what IVF<n>,Flat with these centroids does on add"""
    cent = np.ascontiguousarray(cent, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
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
    return (np.ascontiguousarray(x, dtype=np.float32) - np.ascontiguousarray(cent, dtype=np.float32)[of_row]).astype(np.float32)


def build_lists(metric, cent, cb, x, ids=None):
    """-> per list (stored ids [n_l] int64, codes [n_l, M] uint8) in list order; ids default to the sequence numbers"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    M = cb.shape[0]
    ids = np.arange(x.shape[0], dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    if x.shape[0] == 0:
        return [(np.empty(0, dtype=np.int64), np.empty((0, M), dtype=np.uint8)) for _ in range(cent.shape[0])]
    of_row, rows = assign(metric, cent, x)
    assert (of_row >= 0).all()
    codes = pqr.encode(cb, residuals(cent, x, of_row))
    return [(ids[r], codes[r]) for r in rows]


def train(x, nlist, M, metric):
    """-> (coarse centroids [nlist, d], codebooks [M, 256, dsub])"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    ix = orc.Index(x.shape[1], f"IVF{nlist},Flat", metric)
    ix.train(x)
    cent = ix.ivf_centroids()
    of_row, _ = assign(metric, cent, x)
    return cent, pqr.train_codebooks(residuals(cent, x, of_row), M)


def probes(metric, cent, xq, nprobe):
    """the probed lists of every query in rank order [nq, min(nprobe, nlist)]"""
    _, P = orc.flat_search(metric, np.ascontiguousarray(cent, dtype=np.float32), np.ascontiguousarray(xq, dtype=np.float32), min(nprobe, cent.shape[0]))
    return P


def pair_distances(metric, cent_l, cb, xq, codes):
    """dis [nq, n_l] of the queries against one list's codes"""
    xq = np.ascontiguousarray(xq, dtype=np.float32)
    if metric == L2:
        return pqr.distances(pqr.tables(cb, (xq - cent_l).astype(np.float32), L2), codes)
    T = pqr.tables(cb, xq, IP)
    base = orc.pair_chains(IP, np.ascontiguousarray(cent_l[None], dtype=np.float32), xq)  # [nq, 1]: the chain <x, c>
    dis = np.repeat(base.astype(np.float32), codes.shape[0], axis=1)
    for m in range(cb.shape[0]):
        dis = (dis + T[:, m, :][:, codes[:, m]]).astype(np.float32)
    return dis


def all_pair_distances(metric, cent, cb, lists, xq):
    """per list dis [nq, n_l] of EVERY query against it (None for an empty list): a pair's sum does not depend on its probe rank, so
    tests compute this once and select from it for every (nprobe, k, batch) they try"""
    return [pair_distances(metric, cent[l], cb, xq, codes_l) if ids_l.size else None for l, (ids_l, codes_l) in enumerate(lists)]


def select(metric, P, lists, dis_lists, k, id_map=None, keep_ids=None):
    """P [nq, np]: the probed lists in rank order (-1: none); dis_lists as all_pair_distances gives them (rows of the same queries) ->
    of the values the heap rule admits the k best per query in the pure order (distance, probe rank, position in the list), padded with -1 / +-FLT_MAX.
    id_map: stored id -> label (IDMap); keep_ids: the labels a selector admits"""
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


def search(metric, cent, cb, lists, xq, k, nprobe, id_map=None, keep_ids=None):
    xq = np.ascontiguousarray(xq, dtype=np.float32)
    return select(metric, probes(metric, cent, xq, nprobe), lists, all_pair_distances(metric, cent, cb, lists, xq), k, id_map, keep_ids)


# ---- the IwPQ file (FAISS impl/index_write.cpp, restated): the ivf header as IwFl writes it (header, size_t nlist, nprobe, the quantizer
# index, direct map), uint8 by_residual, size_t code_size, ProductQuantizer {size_t d, M, nbits; vector<float> centroids}, the lists
def _header(d, ntotal, trained, metric):
    return struct.pack("<iqqqBi", d, ntotal, 1 << 20, 1 << 20, 1 if trained else 0, metric)


def write_ivfpq(path_or_none, d, metric, cent, cb, lists, nprobe=1, trained=True, id_map=None, by_residual=1, nbits=8, fourcc=b"IwPQ"):
    """cent None: an index whose quantizer is still empty"""
    M = cb.shape[0]
    nlist = len(lists)
    ntotal = sum(int(i.size) for i, _ in lists)
    body = fourcc + _header(d, ntotal, trained, metric) + struct.pack("<QQ", nlist, nprobe)
    rows = np.empty(0, dtype="<f4") if cent is None else np.ascontiguousarray(cent, dtype="<f4").reshape(-1)
    body += (b"IxF2" if metric == L2 else b"IxFI") + _header(d, rows.size // d, True, metric) + struct.pack("<Q", rows.size) + rows.tobytes()
    body += struct.pack("<bQ", 0, 0)  # DirectMap::NoMap, empty array
    cbf = np.ascontiguousarray(cb, dtype="<f4").reshape(-1)
    body += struct.pack("<BQ", by_residual, M) + struct.pack("<QQQ", d, M, nbits) + struct.pack("<Q", cbf.size) + cbf.tobytes()
    body += b"ilar" + struct.pack("<QQ", nlist, M)
    sizes = [int(i.size) for i, _ in lists]
    if sum(1 for s in sizes if s) > nlist // 2:
        body += b"full" + struct.pack("<Q", nlist) + struct.pack(f"<{nlist}Q", *sizes)
    else:
        flat = [v for l, s in enumerate(sizes) if s for v in (l, s)]
        body += b"sprs" + struct.pack("<Q", len(flat)) + struct.pack(f"<{len(flat)}Q", *flat)
    for ids_l, codes_l in lists:
        if ids_l.size:
            body += np.ascontiguousarray(codes_l, dtype=np.uint8).reshape(-1, M).tobytes() + np.ascontiguousarray(ids_l, dtype="<i8").tobytes()
    if id_map is not None:
        id_map = np.ascontiguousarray(id_map, dtype="<i8")
        body = b"IxMp" + _header(d, ntotal, trained, metric) + body + struct.pack("<Q", id_map.size) + id_map.tobytes()
    if path_or_none is not None:
        with open(path_or_none, "wb") as f:
            f.write(body)
    return body


def parse_ivfpq(buf):
    """-> dict(d, ntotal, trained, metric, nlist, nprobe, centroids [nlist or 0, d], by_residual, code_size, M, nbits,
    codebooks [M, 256, dsub], lists [(ids, codes)], id_map | None)"""
    if not isinstance(buf, (bytes, bytearray)):
        buf = open(buf, "rb").read()
    pos = 0

    def take(fmt):
        nonlocal pos
        v = struct.unpack_from(fmt, buf, pos)
        pos += struct.calcsize(fmt)
        return v

    def array(dtype, count):
        nonlocal pos
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=pos).copy()
        pos += a.nbytes
        return a

    def header():
        d, ntotal, _, _, trained, metric = take("<iqqqBi")
        assert metric <= 1
        return d, ntotal, bool(trained), metric

    cc = bytes(take("<4s")[0])
    wrapped = cc == b"IxMp"
    if wrapped:
        header()
        cc = bytes(take("<4s")[0])
    assert cc == b"IwPQ", cc
    d, ntotal, trained, metric = header()
    nlist, nprobe = take("<QQ")
    qcc = bytes(take("<4s")[0])
    assert qcc in (b"IxF2", b"IxFI", b"IxFl"), qcc
    qd, qn, _, _ = header()
    assert qd == d
    (nf,) = take("<Q")
    assert nf == qn * d
    cent = array("<f4", nf).reshape(-1, d)
    dm_type, dm_n = take("<bQ")
    assert dm_type == 0 and dm_n == 0
    by_residual, code_size = take("<BQ")
    d2, M, nbits = take("<QQQ")
    assert d2 == d
    (ncb,) = take("<Q")
    cb = array("<f4", ncb).reshape(M, 1 << nbits, d // M)
    assert bytes(take("<4s")[0]) == b"ilar"
    nl2, cs2 = take("<QQ")
    assert nl2 == nlist and cs2 == code_size
    kind = bytes(take("<4s")[0])
    (ns,) = take("<Q")
    raw = array("<u8", ns)
    sizes = np.zeros(nlist, dtype=np.int64)
    if kind == b"full":
        assert ns == nlist
        sizes[:] = raw
    else:
        assert kind == b"sprs", kind
        sizes[raw[0::2].astype(np.int64)] = raw[1::2]
    lists = []
    for l in range(nlist):
        codes = array(np.uint8, int(sizes[l]) * code_size).reshape(-1, code_size)
        lists.append((array("<i8", int(sizes[l])), codes))
    id_map = None
    if wrapped:
        (nid,) = take("<Q")
        id_map = array("<i8", nid)
    assert pos == len(buf), (pos, len(buf))
    return dict(d=d, ntotal=ntotal, trained=trained, metric=metric, nlist=nlist, nprobe=nprobe, centroids=cent, by_residual=by_residual,
                code_size=code_size, M=M, nbits=nbits, codebooks=cb, lists=lists, id_map=id_map)
