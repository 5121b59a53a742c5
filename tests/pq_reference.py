"""CPU model of the PQ<M> index (include/mi355_faiss.h "product-quantised indexes"), built on the unchanged oracle, and an
independent writer / parser of the IxPq file layout.  A helper module: nothing here is collected."""
import struct

import numpy as np

from admission_rule import admitted
from oracle import oracle as orc

KSUB = 256
FLT_MAX = np.finfo(np.float32).max


def train_codebooks(x, M):
    """codebook m = the centroids IVF256,Flat (L2) learns from columns [m dsub, (m+1) dsub) -> [M, 256, dsub]"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    d = x.shape[1]
    dsub = d // M
    cb = np.empty((M, KSUB, dsub), dtype=np.float32)
    for m in range(M):
        ix = orc.Index(dsub, "IVF256,Flat", orc.METRIC_L2)
        ix.train(np.ascontiguousarray(x[:, m * dsub : (m + 1) * dsub]))
        cb[m] = ix.ivf_centroids()
    return cb


def synthetic_codebooks(rng, M, dsub, duplicates=True):
    """codebooks that need no k-means; a few duplicated centroids so that the encoder's smallest-j rule matters"""
    cb = rng.standard_normal((M, KSUB, dsub)).astype(np.float32)
    if duplicates:
        cb[:, 200] = cb[:, 17]
        cb[:, 255] = cb[:, 0]
    return cb


def encode(cb, x):
    """code[i][m] = nearest centroid by the pair-path L2 chain, smallest j on a tie -> [n, M] uint8"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    M, _, dsub = cb.shape
    codes = np.empty((x.shape[0], M), dtype=np.uint8)
    for m in range(M):
        _, I = orc.flat_search(orc.METRIC_L2, cb[m], np.ascontiguousarray(x[:, m * dsub : (m + 1) * dsub]), 1, force_path=orc.PATH_PAIR)
        codes[:, m] = I[:, 0].astype(np.uint8)
    return codes


def tables(cb, xq, metric):
    """T[q][m][j]: pair-path L2 or the canonical ip chain between query sub-vector m and centroid j -> [nq, M, 256].  The chains are
    evaluated directly (oracle pair_chains), so a query may hold NaN, inf or values whose squares overflow"""
    xq = np.ascontiguousarray(xq, dtype=np.float32)
    M, _, dsub = cb.shape
    T = np.empty((xq.shape[0], M, KSUB), dtype=np.float32)
    for m in range(M):
        T[:, m, :] = orc.pair_chains(metric, cb[m], np.ascontiguousarray(xq[:, m * dsub : (m + 1) * dsub]))
    return T


def tables_by_search(cb, xq, metric):
    """the same values read off the oracle's k = 256 search of every codebook: finite input only (the search applies the heap's admission
    rule to the entries).  tests/test_admission_rule_cpu.py holds tables() to it bit for bit"""
    xq = np.ascontiguousarray(xq, dtype=np.float32)
    M, _, dsub = cb.shape
    T = np.empty((xq.shape[0], M, KSUB), dtype=np.float32)
    rows = np.arange(xq.shape[0])[:, None]
    for m in range(M):
        D, I = orc.flat_search_naive(metric, cb[m], np.ascontiguousarray(xq[:, m * dsub : (m + 1) * dsub]), KSUB, orc.PATH_PAIR)
        assert (np.sort(I, axis=1) == np.arange(KSUB)).all()
        T[rows, m, I] = D
    return T


def distances(T, codes):
    """dis(q, i) = ((T[q][0][c_i0] + T[q][1][c_i1]) + ...) in f32, m ascending -> [nq, n]"""
    nq, M, _ = T.shape
    dis = T[:, 0, :][:, codes[:, 0]].astype(np.float32)
    for m in range(1, M):
        dis = (dis + T[:, m, :][:, codes[:, m]]).astype(np.float32)
    return dis


def select(dis, k, metric, labels=None, keep=None):
    """dis [nq, n] -> of the values the heap rule admits (tests/admission_rule.py) the k best per query in the pure order (distance, then
    internal row), padded with -1 / +-FLT_MAX; labels: id_map; keep: bool mask over rows (selector)"""
    nq, n = dis.shape
    l2 = metric == orc.METRIC_L2
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


def search(cb, codes, xq, k, metric, labels=None, keep=None):
    T = tables(cb, xq, metric)
    if codes.shape[0] == 0:
        return select(np.empty((T.shape[0], 0), dtype=np.float32), k, metric)
    return select(distances(T, codes), k, metric, labels, keep)


# ---- the IxPq file (FAISS impl/index_write.cpp, restated): header, size_t d M nbits, vector<float> centroids, vector<uint8> codes,
# int32 search_type, uint8 encode_signs, int32 polysemous_ht
def _header(d, ntotal, trained, metric):
    return struct.pack("<iqqqBi", d, ntotal, 1 << 20, 1 << 20, 1 if trained else 0, metric)


def write_pq(path_or_none, d, metric, cb, codes, trained=True, ids=None):
    M = cb.shape[0]
    codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1, M)
    n = codes.shape[0]
    cbf = np.ascontiguousarray(cb, dtype="<f4").reshape(-1)
    body = b"IxPq" + _header(d, n, trained, metric)
    body += struct.pack("<QQQ", d, M, 8)
    body += struct.pack("<Q", cbf.size) + cbf.tobytes()
    body += struct.pack("<Q", codes.size) + codes.tobytes()
    body += struct.pack("<iBi", 0, 0, 8 * M + 1)
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype="<i8")
        body = b"IxMp" + _header(d, n, trained, metric) + body + struct.pack("<Q", ids.size) + ids.tobytes()
    if path_or_none is not None:
        with open(path_or_none, "wb") as f:
            f.write(body)
    return body


def parse_pq(buf):
    """-> dict(d, ntotal, trained, metric, M, nbits, centroids [M,256,dsub], codes [n,M], search_type, polysemous_ht, ids | None)"""
    if not isinstance(buf, (bytes, bytearray)):
        buf = open(buf, "rb").read()
    pos = 0

    def take(fmt):
        nonlocal pos
        v = struct.unpack_from(fmt, buf, pos)
        pos += struct.calcsize(fmt)
        return v

    def header():
        d, ntotal, _, _, trained, metric = take("<iqqqBi")
        assert metric <= 1
        return d, ntotal, bool(trained), metric

    cc = bytes(take("<4s")[0])
    ids = None
    wrapped = cc == b"IxMp"
    if wrapped:
        header()
        cc = bytes(take("<4s")[0])
    assert cc == b"IxPq", cc
    d, ntotal, trained, metric = header()
    d2, M, nbits = take("<QQQ")
    assert d2 == d
    (ncb,) = take("<Q")
    cb = np.frombuffer(buf, dtype="<f4", count=ncb, offset=pos).reshape(M, 1 << nbits, d // M).copy()
    pos += 4 * ncb
    (nc,) = take("<Q")
    codes = np.frombuffer(buf, dtype=np.uint8, count=nc, offset=pos).reshape(-1, M).copy()
    pos += nc
    search_type, encode_signs, ht = take("<iBi")
    if wrapped:
        (nid,) = take("<Q")
        ids = np.frombuffer(buf, dtype="<i8", count=nid, offset=pos).copy()
        pos += 8 * nid
    assert pos == len(buf), (pos, len(buf))
    return dict(d=d, ntotal=ntotal, trained=trained, metric=metric, M=M, nbits=nbits, centroids=cb, codes=codes,
                search_type=search_type, encode_signs=encode_signs, polysemous_ht=ht, ids=ids)
