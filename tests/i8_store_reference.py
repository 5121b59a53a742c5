"""The host decisions of the d <= 128 coarse filter's stores restated in numpy (FlatIndex::ensure_h1_rows / ensure_i8_rows of
csrc/flat_coarse.hip, the conversion kernels of csrc/flat_collect.hip, DESIGN.md 3.1 "int8 store"): the centre, the outlier threshold and
the outlier rows, the int8 scales, the format rule, the 2^24 range check -- at the first build and after rows were added -- and the
share of a query batch that clamps.  Sums are float64 where the kernels reduce in float32, so the two agree to a few ulps of the sums and
no further: decided() answers "borderline" wherever that could change the outcome, and a GPU test asserts first that its data is not.

Not a test module: tests/test_collect_i8_bound_cpu.py and tests/test_collect_i8_hostile_gpu.py use it."""

import copy
import math

import numpy as np

L2, IP = 1, 0
MIN_ROWS = 262_144  # the smallest store that gets an outlier threshold, and an int8 store
MEAN_ROWS = 1 << 20  # the centre is the mean of at most this many rows
_CHUNK = 32_768
# How near the format rule's threshold 4 the ratio e_i8 / e_bf16 may come before decided() calls it borderline.  Both terms are maxima of
# sums of squares that depend on the data and, continuously, on the centre; the device's float32 centre and sums agree with the float64
# ones here to about 1e-4 relative (2^20 terms of like sign, pairwise within a block), so 3 % is some hundred times what could differ.
# (Uniform rows sit at 2.1 ... 2.4 for every 17 <= d <= 128: a band of a factor two would call the store's everyday input borderline.)
RATIO_BAND = 1.03


def bf16_round(v):
    """float32 -> the nearest bfloat16 (ties to even), as float32"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    r = (u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def _rowsum(a):
    """row sums of squares of a float32 array, accumulated in float64"""
    return np.einsum("ij,ij->i", a, a, dtype=np.float64)


class StoreModel:
    """rows: every row the index ever holds, in arrival order ([n, d] float32); n_first: the rows present when the coarse filter's store
    is first built (the first search through it); n_i8: the rows present at the first search the int8 store may serve (>= 262 144 rows,
    a batch beyond the small-batch path) -- n_first by default."""

    def __init__(self, rows, n_first, metric, n_i8=None):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n, d = rows.shape
        self.n, self.d = n, d
        self.n_first = int(n_first)
        self.n_i8 = int(n_first if n_i8 is None else n_i8)
        assert 0 < self.n_first <= self.n_i8 <= n  # (the device also wants n_i8 >= MIN_ROWS; the rule itself does not depend on it)
        nm = min(self.n_first, MEAN_ROWS)
        self.mu = rows[:nm].mean(0, dtype=np.float64)
        mu32 = self.mu.astype(np.float32)
        # per row: ||y'||^2 (y' = y - mu in float32, as the kernels centre), ||y||^2, max |y'_i|, ||y' - bf16(y')||^2, <mu, y>
        self.n2, self.yn = np.empty(n), np.empty(n)
        self.amax_row, self.res_bf_row, self.my = np.empty(n), np.empty(n), np.empty(n)
        for i0 in range(0, n, _CHUNK):
            s = slice(i0, min(n, i0 + _CHUNK))
            y = rows[s]
            c = y - mu32
            self.n2[s] = _rowsum(c)
            self.yn[s] = _rowsum(y)
            self.amax_row[s] = np.abs(c).max(1)
            self.res_bf_row[s] = _rowsum(c - bf16_round(c))  # (the difference is exact in float32: the two agree in their leading 8 bits)
            self.my[s] = np.einsum("ij,j->i", y, mu32, dtype=np.float64)
        # tau = 64 x the mean ||y - mu||^2 of the rows the centre was averaged over; only stores of >= 262 144 rows at the first build
        self.tau = math.inf
        if self.n_first >= MIN_ROWS:
            mean_c = float(self.yn[:nm].mean() - (self.mu**2).sum())
            if 0.0 < mean_c < 1e30:
                self.tau = 64.0 * mean_c
        self.is_outlier = self.n2 > self.tau
        self.outliers = np.flatnonzero(self.is_outlier)
        # the scales, from the rows of the first int8 build that are in the store
        first = ~self.is_outlier[: self.n_i8]
        self.amax = float(self.amax_row[: self.n_i8][first].max()) if first.any() else 0.0
        self.valid = 0.0 < self.amax < 1e30
        self.metric = None
        if not self.valid:
            self._set_metric(metric)
            return
        self.sy_exp = math.log2(self.amax / (128.0 * 1.01))
        self.sy = 2.0 ** math.ceil(self.sy_exp)
        self.limit = float((1 << 23) - d * 16384)
        self.res_i8_row = np.empty(n)
        for i0 in range(0, n, _CHUNK):
            s = slice(i0, min(n, i0 + _CHUNK))
            c = rows[s] - mu32
            q = np.clip(np.rint(c * np.float32(1.0 / self.sy)), -128, 127)
            self.res_i8_row[s] = _rowsum(c - np.float32(self.sy) * q)  # (float32, as the kernel: exact where nothing clamps)
        self.res_i8 = float(self.res_i8_row[: self.n_i8][first].max())
        self.res_bf = float(self.res_bf_row[: self.n_i8][first].max())
        self._set_metric(metric)

    def _set_metric(self, metric):
        self.metric = metric
        self.alpha = 2.0 if metric == L2 else 1.0
        self.beta = -self.n2 if metric == L2 else self.my
        if not self.valid:
            return
        self.sa = self.alpha * self.sy
        self.unit = self.alpha * self.sy * self.sy
        self.beta_int = np.abs(np.rint(self.beta / self.unit))
        # the format rule, once, at the first int8 build
        self.e_i8 = self.sa * math.sqrt(self.d / 12.0) + self.alpha * math.sqrt(self.res_i8)
        self.e_bf = 2.0 * self.alpha * math.sqrt(self.res_bf)
        self.ratio = self.e_i8 / self.e_bf if self.e_bf > 0 else math.inf

    def with_metric(self, metric):
        """the same rows under the other metric (everything but alpha and beta is shared)"""
        if metric == self.metric:
            return self
        m = copy.copy(self)
        m._set_metric(metric)
        return m

    def beta_max(self, n=None):
        """max |beta_int| over the rows in the store when the index holds its first n rows (all by default): against limit = 2^23 - d 2^14"""
        n = self.n if n is None else n
        keep = ~self.is_outlier[:n]
        return float(self.beta_int[:n][keep].max()) if keep.any() else 0.0

    def residual_max(self, n=None):
        """max ||y' - sy Y||^2 over the same rows: the bound's row residual, clamped components included"""
        n = self.n if n is None else n
        keep = ~self.is_outlier[:n]
        return float(self.res_i8_row[:n][keep].max()) if keep.any() else 0.0

    def outlier_rows(self, n=None):
        n = self.n if n is None else n
        return self.outliers[self.outliers < n]

    def clamped_share(self, xq):
        """the share of the queries with at least one component of alpha (x - mu) beyond +-128 sa"""
        a = np.float32(self.alpha) * (np.asarray(xq, dtype=np.float32) - self.mu.astype(np.float32))
        t = np.rint(a * np.float32(1.0 / self.sa))
        return float(((t > 127) | (t < -128)).any(1).mean())

    def decided(self, n=None):
        """"int8" | "bf16": the store that serves an index holding the first n rows (all by default; n >= n_i8), searched at n_i8 rows first;
        "borderline": float32 sums on the device could decide otherwise"""
        n = self.n if n is None else n
        assert n >= self.n_i8
        if not self.valid:
            return "bf16"  # (amax = 0: nothing to scale by)
        near = self.n2[:n][(self.n2[:n] > 0.8 * self.tau) & (self.n2[:n] < 1.25 * self.tau)]
        if near.size:  # (a row near the outlier threshold -- the device's is a mean over every 16th row -- is in or out of the store and of every maximum)
            return "borderline"
        if abs(self.sy_exp - round(self.sy_exp)) < 1e-3:  # (amax at a power of two: sy could come out twice or half as large)
            return "borderline"
        if 4.0 / RATIO_BAND < self.ratio < 4.0 * RATIO_BAND:
            return "borderline"
        b_first, b_all = self.beta_max(self.n_i8), self.beta_max(n)
        for b in (b_first, b_all):
            if 0.9 * self.limit < b < 1.1 * self.limit:
                return "borderline"
        if self.ratio > 4.0 or not b_first < self.limit:
            return "bf16"  # declined at the first build
        return "int8" if b_all < self.limit else "bf16"  # (a later row broke the range: the store is dropped)

    def describe(self, n=None):
        if not self.valid:
            return "amax = %g: no int8 store" % self.amax
        return "sy = 2^%d, e_i8 / e_bf16 = %.3g / %.3g = %.3g (<= 4), max |beta_int| = %.4g (< %.4g), tau = %.4g, %d outlier rows -> %s" % (
            round(math.log2(self.sy)), self.e_i8, self.e_bf, self.ratio, self.beta_max(n), self.limit, self.tau,
            self.outlier_rows(n).size, self.decided(n))  # fmt: skip


def decided(rows, n_first, metric, n_i8=None, n=None):
    return StoreModel(rows, n_first, metric, n_i8).decided(n)
