"""numpy float32 model of IndexIVFPQFastScan (include/mi355_faiss.h "inverted lists of 4-bit product-quantised residuals") on
integer-valued data, where every f32 chain is exact in any order of summation: only the contract's division, fmaf and floor remain.
Built on tests/ivfpq_reference.py (assignment, probes, the pure order).  A helper module: nothing here is collected."""
import functools

import numpy as np

import ivfpq_reference as ivr

L2, IP = ivr.L2, ivr.IP


def tables(cb, v, metric):
    """T[i][m][j] of vectors v [n, d] against codebooks cb [M, 16, dsub] -> [n, M, 16] f32"""
    M, _, dsub = cb.shape
    vs = v.reshape(v.shape[0], M, 1, dsub)
    return (((vs - cb[None]) ** 2) if metric == L2 else vs * cb[None]).sum(-1, dtype=np.float32)


def encode(cb, res):
    return tables(cb, res, L2).argmin(2).astype(np.uint8)  # (the first minimum: the smallest j)


def pack(codes):
    """FAISS's packing: the code of an even m in the low nibble of byte m / 2"""
    return codes[:, 0::2] | (codes[:, 1::2] << 4)


def decode(cb, codes):
    return cb[np.arange(cb.shape[0])[None, :], codes].reshape(codes.shape[0], -1)


def build_lists(metric, cent, cb, x, ids=None):
    """-> per list (stored ids, codes [n_l, M]) in list order"""
    ids = np.arange(x.shape[0], dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    of_row, rows = ivr.assign(metric, cent, x)
    codes = encode(cb, ivr.residuals(cent, x, of_row))
    return [(ids[r], codes[r]) for r in rows]


@np.errstate(all="ignore")
def pair_distances(metric, cent_l, cb, xq, codes):
    """dis [nq, n_l] of every query against one list; a pair with a non-finite table entry or base contributes no row: NaN, which the
    admission rule drops"""
    v = (xq - cent_l).astype(np.float32) if metric == L2 else xq
    T = tables(cb, v, metric)
    base = np.zeros(xq.shape[0], dtype=np.float32) if metric == L2 else (xq * cent_l).sum(1, dtype=np.float32)
    lo, hi = T.min(2), T.max(2)
    span = (hi - lo).max(1)
    a = np.divide(np.float32(255), span, out=np.zeros_like(span), where=span != 0)
    b = functools.reduce(lambda s, m: s + lo[:, m], range(lo.shape[1]), base)
    # fmaf(T - lo, a, 0.5f): the product and the sum are exact in double, so one rounding to f32
    tq = np.floor(((T - lo[:, :, None]).astype(np.float64) * a[:, None, None] + 0.5).astype(np.float32)).clip(0, 255).astype(np.int64)
    s = sum(tq[:, m, :][:, codes[:, m]] for m in range(codes.shape[1])).astype(np.float32)
    dis = np.where(a[:, None] != 0, b[:, None] + s / np.where(a != 0, a, 1)[:, None], b[:, None]).astype(np.float32)
    dis[~(np.isfinite(T).all((1, 2)) & np.isfinite(base))] = np.nan
    return dis


def all_pair_distances(metric, cent, cb, lists, xq):
    return [pair_distances(metric, cent[l], cb, xq, c) if i.size else None for l, (i, c) in enumerate(lists)]


def search(metric, cent, cb, lists, dis_lists, xq, k, nprobe, keep_ids=None):
    """dis_lists: all_pair_distances of the same queries.  A query with a NaN or inf component has no valid pair: only missing slots"""
    D = np.full((xq.shape[0], k), ivr.FLT_MAX if metric == L2 else -ivr.FLT_MAX, dtype=np.float32)
    I = np.full((xq.shape[0], k), -1, dtype=np.int64)
    ok = np.flatnonzero(np.isfinite(xq).all(1))
    P = ivr.probes(metric, cent, xq[ok], nprobe)
    sub = [None if dl is None else dl[ok] for dl in dis_lists]
    D[ok], I[ok] = ivr.select(metric, P, lists, sub, k, keep_ids=keep_ids)
    return D, I
