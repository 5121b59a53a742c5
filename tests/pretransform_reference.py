"""CPU model of the pre-transform indexes (include/mi355_faiss.h "pre-transform indexes"): the linear transform as the oracle's pair-path chains
plus one f32 addition, L2norm in numpy f32 over the same chains, PCA by numpy.linalg.eigh in f64 with the header's order, sign, rounding and
bias rules, and a writer / parser of the "IxPT" image.  Nothing here runs on the device."""
import struct

import numpy as np

import sq_reference as sqr
from oracle import oracle as orc

L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
VT_LINEAR, VT_PCA, VT_NORM = 0, 1, 2
LINEAR_FOURCCS = (b"LTra", b"rrot", b"PCAm", b"PcAm")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- apply
def linear(A, b, x):
    """y[i, j] = (acc = fmaf(x[i, k], A[j, k], acc), k ascending from +0) + b[j]; b None: no addition.  A row of x that holds a NaN gives a row
    of NaNs (every chain meets it), which the oracle's sort is not asked to order"""
    A, x = _f32(A), _f32(x)
    n, dout = x.shape[0], A.shape[0]
    y = np.full((n, dout), np.nan, dtype=np.float32)
    ok = ~np.isnan(x).any(axis=1)
    if ok.any():
        y[ok] = sqr.chains(IP, A, x[ok])
    if b is not None:
        y = (y + _f32(b)[None, :]).astype(np.float32)
    return y


def sqnorm_chains(x):
    """nr[i] = (acc = fmaf(x[i, k], x[i, k], acc), k ascending from +0); NaN for a row that holds one"""
    x = _f32(x)
    nr = np.full(x.shape[0], np.nan, dtype=np.float32)
    ok = ~np.isnan(x).any(axis=1)
    for i0 in range(0, int(ok.sum()), 256):  # (the chains of a block of rows against itself: the diagonal)
        rows = np.flatnonzero(ok)[i0 : i0 + 256]
        nr[rows] = np.diagonal(sqr.chains(IP, x[rows], x[rows]))
    return nr


def l2norm(x):
    """fvec_renorm_L2: nr > 0: y = x * (1 / sqrt(nr)) in f32, every operation rounded once; otherwise (zero or NaN norm) the row is copied"""
    x = _f32(x)
    nr = sqnorm_chains(x)
    y = x.copy()
    with np.errstate(all="ignore"):
        go = nr > 0
        inv = (np.float32(1.0) / np.sqrt(nr[go], dtype=np.float32)).astype(np.float32)
        y[go] = (x[go] * inv[:, None]).astype(np.float32)
    return y


def apply_chain(chain, x):
    """chain: dicts with type VT_NORM, or A and b (None: no bias)"""
    y = _f32(x)
    for t in chain:
        y = l2norm(y) if t["type"] == VT_NORM else linear(t["A"], t.get("b"), y)
    return y


# ---- PCA
def pca_bias(A, mean):
    """b[j] = -sum_k A[j, k] mean[k], accumulated in f64 over the f32 values with k ascending, rounded once"""
    A, mean = _f32(A), _f32(mean)
    acc = np.zeros(A.shape[0], dtype=np.float64)
    for k in range(A.shape[1]):
        acc += A[:, k].astype(np.float64) * np.float64(mean[k])
    return (-acc).astype(np.float32)


def fix_signs(V):
    """rows of V: the component of largest magnitude (the first such) is made positive"""
    V = np.array(V, dtype=np.float64)
    for i in range(V.shape[0]):
        if V[i, int(np.argmax(np.abs(V[i])))] < 0:
            V[i] = -V[i]
    return V


def pca_train(x, d_out, whiten=False):
    x64 = _f32(x).astype(np.float64)
    n, d = x64.shape
    mean = x64.mean(axis=0)
    xc = x64 - mean
    C = xc.T @ xc / n
    lam, vec = np.linalg.eigh(C)
    order = np.argsort(-lam, kind="stable")
    lam, V = lam[order], fix_signs(vec[:, order].T)
    A64 = V[:d_out].copy()
    if whiten:
        assert (lam[:d_out] > 0).all()
        A64 = A64 * (1.0 / np.sqrt(lam[:d_out]))[:, None]
    A = A64.astype(np.float32)
    mean32 = mean.astype(np.float32)
    return dict(type=VT_PCA, d_in=d, d_out=d_out, mean=mean32, eigenvalues=lam.astype(np.float32), PCAMat=V.astype(np.float32), A=A,
                b=pca_bias(A, mean32), lam64=lam, V64=V, C=C)


def planted(seed=7, d=12, n=4096):
    """variances 2^-i along a random orthonormal basis, plus an offset"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    z = rng.standard_normal((n, d)) * np.sqrt(2.0 ** -np.arange(d))[None, :]
    return (z @ Q.T + rng.standard_normal(d)[None, :] * 3.0).astype(np.float32)


def spectrum_gaps(lam):
    """(smallest relative gap, smallest absolute gap) between neighbours of a descending spectrum"""
    lam = np.asarray(lam, dtype=np.float64)
    gap = lam[:-1] - lam[1:]
    return float((gap / lam[:-1]).min()), float(gap.min())


# ---- the "IxPT" image: the index header, int32 n, n transforms, the sub-index's image (IDMap: "IxMp" around the whole, the id map behind it)
def _header(d, ntotal, trained, metric):
    return struct.pack("<iqqqBi", d, ntotal, 1 << 20, 1 << 20, 1 if trained else 0, metric)


def _vec(a):
    a = np.ascontiguousarray(a, dtype="<f4").reshape(-1)
    return struct.pack("<Q", a.size) + a.tobytes()


def transform_bytes(t):
    """t: dict(fourcc, d_in, d_out, is_trained) and, by fourcc, norm | have_bias, A, b [, eigen_power, epsilon, random_rotation, balanced_bins,
    mean, eigenvalues, PCAMat]"""
    cc = t["fourcc"]
    out = cc
    if cc == b"VNrm":
        out += struct.pack("<f", t.get("norm", 2.0))
    elif cc in LINEAR_FOURCCS:
        if cc in (b"PCAm", b"PcAm"):
            out += struct.pack("<f", t.get("eigen_power", 0.0))
            if cc == b"PcAm":
                out += struct.pack("<f", t.get("epsilon", 0.0))
            out += struct.pack("<Bi", 1 if t.get("random_rotation") else 0, t.get("balanced_bins", 0))
            out += _vec(t.get("mean", [])) + _vec(t.get("eigenvalues", [])) + _vec(t.get("PCAMat", []))
        b = t.get("b")
        have_bias = t.get("have_bias", b is not None)
        out += struct.pack("<B", 1 if have_bias else 0) + _vec(t.get("A", [])) + _vec([] if b is None else b)
    # (any other fourcc: nothing of its own -- the images the reader must refuse by name)
    return out + struct.pack("<iiB", t["d_in"], t["d_out"], 1 if t.get("is_trained", True) else 0)


def write_pretransform(path_or_none, d, metric, chain, sub_image, ntotal=0, trained=True, id_map=None):
    body = b"IxPT" + _header(d, ntotal, trained, metric) + struct.pack("<i", len(chain)) + b"".join(transform_bytes(t) for t in chain) + sub_image
    if id_map is not None:
        id_map = np.ascontiguousarray(id_map, dtype="<i8")
        body = b"IxMp" + _header(d, ntotal, trained, metric) + body + struct.pack("<Q", id_map.size) + id_map.tobytes()
    if path_or_none is not None:
        with open(path_or_none, "wb") as f:
            f.write(body)
    return body


def parse_pretransform(buf):
    """-> dict(d, ntotal, trained, metric, chain = [dict], sub = the sub-index's image (bytes), id_map)"""
    pos = 0

    def take(fmt):
        nonlocal pos
        v = struct.unpack_from("<" + fmt, buf, pos)
        pos += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def vec():
        nonlocal pos
        n = take("Q")
        a = np.frombuffer(buf, dtype="<f4", count=n, offset=pos).copy()
        pos += 4 * n
        return a

    def header():
        d, ntotal, _, _, trained, metric = take("iqqqBi")
        return d, ntotal, bool(trained), metric

    cc = buf[:4]
    pos = 4
    idmap = cc == b"IxMp"
    if idmap:
        header()
        cc = buf[pos : pos + 4]
        pos += 4
    assert cc == b"IxPT", cc
    d, ntotal, trained, metric = header()
    chain = []
    for _ in range(take("i")):
        t = dict(fourcc=buf[pos : pos + 4])
        pos += 4
        if t["fourcc"] == b"VNrm":
            t["type"], t["norm"] = VT_NORM, take("f")
        else:
            assert t["fourcc"] in LINEAR_FOURCCS, t["fourcc"]
            t["type"] = VT_LINEAR
            if t["fourcc"] in (b"PCAm", b"PcAm"):
                t["type"] = VT_PCA
                t["eigen_power"] = take("f")
                if t["fourcc"] == b"PcAm":
                    t["epsilon"] = take("f")
                t["random_rotation"], t["balanced_bins"] = take("Bi")
                t["mean"], t["eigenvalues"], t["PCAMat"] = vec(), vec(), vec()
            t["have_bias"] = bool(take("B"))
            t["A"], t["b"] = vec(), vec()
        t["d_in"], t["d_out"], tr = take("iiB")
        t["is_trained"] = bool(tr)
        if t["type"] != VT_NORM and t["A"].size == t["d_in"] * t["d_out"]:
            t["A"] = t["A"].reshape(t["d_out"], t["d_in"])
        chain.append(t)
    end = len(buf)
    id_map = None
    if idmap:  # the id map is the image's tail: a u64 count and that many int64
        end = len(buf) - 8 * ntotal - 8
        assert struct.unpack_from("<Q", buf, end)[0] == ntotal
        id_map = np.frombuffer(buf, dtype="<i8", count=ntotal, offset=end + 8).copy()
    return dict(d=d, ntotal=ntotal, trained=trained, metric=metric, chain=chain, sub=bytes(buf[pos:end]), id_map=id_map)
