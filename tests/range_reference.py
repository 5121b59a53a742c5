"""CPU model of range search (include/mi355_faiss.h "range search") on the unchanged oracle.  Not collected.

Every distance of either Flat branch comes from orc.flat_search_naive with k = n (PATH_PAIR: the per-pair chains; PATH_BLAS: the value
(xn + yn) - 2 ip clamped at 0); the two L2 branches differ bitwise in most slots, so a kernel on the wrong branch cannot pass.  For inner
product both branches are the same chain.  The IVF model takes its lists from orc.Index("IVF<n>,Flat") and the probed lists from the
oracle's Flat search over the centroids (tests/sq_reference.py probes), or from the caller."""
import numpy as np

from oracle import oracle as orc

L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def all_distances(metric, rows, xq, path):
    """[nq, n] every distance of one branch (orc.PATH_PAIR | orc.PATH_BLAS)"""
    rows, xq = _f32(rows), _f32(xq)
    n = rows.shape[0]
    out = np.empty((xq.shape[0], n), dtype=np.float32)
    if n == 0 or xq.shape[0] == 0:
        return out
    D, I = orc.flat_search_naive(metric, rows, xq, n, path)
    assert (np.sort(I, axis=1) == np.arange(n)).all()
    out[np.arange(xq.shape[0])[:, None], I] = D
    return out


def flat_branch(nq, has_sel):
    """FlatIndex::search_flat's dispatch: a selector or fewer than 20 queries -> the per-pair chains, else the BLAS-branch value"""
    return orc.PATH_PAIR if (has_sel or nq < 20) else orc.PATH_BLAS


def flat_matrix(metric, rows, xq, has_sel=False):
    return all_distances(metric, rows, xq, flat_branch(_f32(xq).shape[0], has_sel))


def hits(metric, dis, radius):
    """strict; False for a NaN distance and for a NaN radius (numpy's comparisons are IEEE's)"""
    with np.errstate(invalid="ignore"):
        return dis < np.float32(radius) if metric == L2 else dis > np.float32(radius)


def select(metric, dis, radius, labels=None, keep=None, label_offset=0):
    """dis [nq, n] -> (lims, D, I): per query the hits in ascending row order; labels: id_map; keep: bool mask over rows"""
    nq, n = dis.shape
    h = hits(metric, dis, radius)
    if keep is not None:
        h = h & np.asarray(keep, dtype=bool)[None, :]
    lims = np.zeros(nq + 1, dtype=np.int64)
    lims[1:] = np.cumsum(h.sum(1))
    q, r = np.nonzero(h)  # row-major: ascending query, then ascending row
    D = dis[q, r].astype(np.float32)
    I = (r.astype(np.int64) + label_offset) if labels is None else np.asarray(labels, dtype=np.int64)[r]
    return lims, D, I


def flat_range(metric, rows, xq, radius, labels=None, keep=None, label_offset=0):
    return select(metric, flat_matrix(metric, rows, xq, keep is not None), radius, labels, keep, label_offset)


# ---- IVF<n>,Flat
def build_lists(metric, cent, x, ids=None):
    """-> per list (stored ids [n_l] int64, rows [n_l, d] f32) in list order: what IVF<n>,Flat with these centroids holds after add"""
    cent, x = _f32(cent), _f32(x)
    nlist, d = cent.shape
    ix = orc.Index(d, f"IVF{nlist},Flat", metric)
    ix.ivf_set_centroids(cent)
    if x.shape[0]:
        ix.add_with_ids(x, np.arange(x.shape[0], dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64))
    return [ix.ivf_list(l) for l in range(nlist)]


def probes(metric, cent, xq, nprobe):
    """the probed lists of every query in rank order [nq, min(nprobe, nlist)]: the Flat quantiser's own search (its dispatch included)"""
    _, P = orc.flat_search(metric, _f32(cent), _f32(xq), min(nprobe, cent.shape[0]))
    return P


def ivf_range(metric, lists, P, xq, radius, id_map=None, keep_ids=None):
    """P [nq, np] probed lists (-1: none).  Per query the rows of the probed lists whose per-pair chain against the raw row passes, in
    (probe rank, position) order.  id_map: dict-like / array from stored id to label; keep_ids: set of ids (the external ones under IDMap)
    the selector keeps"""
    xq = _f32(xq)
    nq = xq.shape[0]
    dis = [all_distances(metric, rows, xq, orc.PATH_PAIR) for _, rows in lists]
    lims, D, I = np.zeros(nq + 1, dtype=np.int64), [], []
    for q in range(nq):
        cnt = 0
        for l in P[q]:
            if l < 0:
                continue
            ids = lists[l][0]
            lab = ids if id_map is None else np.asarray(id_map, dtype=np.int64)[ids]
            h = hits(metric, dis[l][q], radius)
            if keep_ids is not None:
                h = h & np.isin(lab, np.asarray(sorted(keep_ids), dtype=np.int64))
            D.append(dis[l][q][h])
            I.append(lab[h])
            cnt += int(h.sum())
        lims[q + 1] = lims[q] + cnt
    D = np.concatenate(D).astype(np.float32) if D else np.empty(0, dtype=np.float32)
    I = np.concatenate(I).astype(np.int64) if I else np.empty(0, dtype=np.int64)
    return lims, D, I


def same(a, b):
    """(lims, D, I) equal: labels and lims as integers, distances as bit patterns"""
    return (np.array_equal(a[0], b[0]) and np.array_equal(np.asarray(a[2]), np.asarray(b[2]))
            and np.array_equal(_f32(a[1]).view(np.uint32), _f32(b[1]).view(np.uint32)))
