"""bfKnn against a half-precision Flat clone of the same rows, the copy-and-clone route and torch.

  python tools/bfknn_bench.py --out profiles/bfknn_bench.txt [--n 10000000] [--d 128] [--k 10] [--dtype bf16]

Per (layout, nq): median of 5 searches after 2 warm-ups, HIP events, bfKnn and the Flat16 clone alternating.  Flat16's code is what the
parent commit had, so it is the yardstick.  Then the route a caller had before: widen to f32, add to Flat, clone with use_float16,
search (wall time, once).  Then torch on the same half tensors: matmul + topk, chunked over rows."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))
import mi355_faiss as mf  # noqa: E402

F16_PEAK, HBM_PEAK = 2500e12, 8e12  # dense f16 matrix FLOP/s and HBM bytes/s of the part's data sheet


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def torch_knn(xb, xq, k, metric, chunk=1 << 20):
    best_d = best_i = None
    qn = (xq.float() ** 2).sum(1, keepdim=True)
    for r0 in range(0, xb.shape[0], chunk):
        blk = xb[r0 : r0 + chunk]
        s = (xq @ blk.t()).float()
        if metric == mf.METRIC_L2:
            s = qn + (blk.float() ** 2).sum(1)[None, :] - 2 * s
        dd, ii = torch.topk(s, k, dim=1, largest=metric != mf.METRIC_L2)
        ii += r0
        if best_d is not None:
            dd, ii = torch.cat([best_d, dd], 1), torch.cat([best_i, ii], 1)
            dd, sel = torch.topk(dd, k, dim=1, largest=metric != mf.METRIC_L2)
            ii = torch.gather(ii, 1, sel)
        best_d, best_i = dd, ii
    return best_d, best_i


def bf16_against_f16(n, d, k, metric):
    """--dtype bf16: bfKnn over the bf16 copy of the rows beside bfKnn over the fp16 copy, same build, alternating"""
    lines = ["# tools/bfknn_bench.py --dtype bf16 --n %d --d %d --k %d" % (n, d, k),
             "# %s, %s, uniform rows, L2; median of 5 after 2 warm-ups (HIP events), bfKnn over bf16 and over fp16 rows alternating"
             % (time.strftime("%Y-%m-%d"), torch.cuda.get_device_name(0)),
             "%-10s %6s %12s %12s %10s" % ("layout", "nq", "bf16 ms", "fp16 ms", "ratio")]
    x32 = mf.synth_uniform_torch(n, d, 1)
    xh, xb = x32.half(), x32.bfloat16()
    del x32
    torch.cuda.empty_cache()
    mats = (("row-major", xh, xb), ("col-major", xh.t().contiguous().t(), xb.t().contiguous().t()))
    for nq in (10000, 16):
        xq = mf.synth_uniform_torch(nq, d, 2)
        for name, vh, vb in mats:
            D, I = mf.bf_knn_torch(vb, xq, k, metric)
            for _ in range(2):
                mf.bf_knn_torch(vb, xq, k, metric, D=D, I=I)
                mf.bf_knn_torch(vh, xq, k, metric, D=D, I=I)
            rb, rh = [], []
            for _ in range(5):
                rb.append(timed(lambda: mf.bf_knn_torch(vb, xq, k, metric, D=D, I=I), reps=1, warm=0)[0])
                rh.append(timed(lambda: mf.bf_knn_torch(vh, xq, k, metric, D=D, I=I), reps=1, warm=0)[0])
            tb, th = float(np.median(rb)), float(np.median(rh))
            lines.append("%-10s %6d %12.2f %12.2f %10.2f   (bf16 min %.2f max %.2f, fp16 min %.2f max %.2f)"
                         % (name, nq, tb, th, tb / th, min(rb), max(rb), min(rh), max(rh)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--dtype", choices=("f16", "bf16"), default="f16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, d, k, metric = a.n, a.d, a.k, mf.METRIC_L2
    if a.dtype == "bf16":
        text = "\n".join(bf16_against_f16(n, d, k, metric)) + "\n"
        print(text)
        if a.out:
            open(a.out, "a").write(text)  # (appended: the fp16 figures of the file stay)
        return
    lines = ["# tools/bfknn_bench.py --n %d --d %d --k %d" % (n, d, k),
             "# %s, %s, uniform rows, L2; median of 5 after 2 warm-ups (HIP events), bfKnn and the Flat16 clone alternating"
             % (time.strftime("%Y-%m-%d"), torch.cuda.get_device_name(0))]
    x32 = mf.synth_uniform_torch(n, d, 1)
    t0 = time.perf_counter()  # the route a caller had: the f32 matrix exists already (widening a half tensor is x16.float())
    src = mf.index_factory(d, "Flat", metric)
    src.add_torch(x32)
    f16 = src.clone_to_gpu(0, use_float16=True)
    torch.cuda.synchronize()
    t_build = (time.perf_counter() - t0) * 1e3
    del src
    x16 = x32.half()
    t0 = time.perf_counter()
    _ = x16.float()
    torch.cuda.synchronize()
    t_widen = (time.perf_counter() - t0) * 1e3
    del x32, _
    torch.cuda.empty_cache()
    x16c = x16.t().contiguous().t()  # the same values, column-major
    lines.append("%-10s %6s %12s %12s %10s %12s %14s" % ("layout", "nq", "bfKnn ms", "Flat16 ms", "ratio", "of f16 peak", "rows bytes/s"))
    for nq in (10000, 16):
        xq = mf.synth_uniform_torch(nq, d, 2)
        Df, If = f16.search_torch(xq, k)
        for name, xb in (("row-major", x16), ("col-major", x16c)):
            D, I = mf.bf_knn_torch(xb, xq, k, metric)
            same = bool((I == If).all()) and bool((D.view(torch.int32) == Df.view(torch.int32)).all())
            tb = timed(lambda: mf.bf_knn_torch(xb, xq, k, metric, D=D, I=I), reps=1, warm=1)  # (first alternation: warm both)
            tf = timed(lambda: f16.search_torch(xq, k, D=Df, I=If), reps=1, warm=1)
            rb, rf = [], []
            for _ in range(5):
                rb.append(timed(lambda: mf.bf_knn_torch(xb, xq, k, metric, D=D, I=I), reps=1, warm=0)[0])
                rf.append(timed(lambda: f16.search_torch(xq, k, D=Df, I=If), reps=1, warm=0)[0])
            tb, tf = float(np.median(rb)), float(np.median(rf))
            lines.append("%-10s %6d %12.2f %12.2f %10.2f %11.1f%% %14.3e   (bfKnn min %.2f max %.2f, Flat16 min %.2f max %.2f; same bits as Flat16: %s)"
                         % (name, nq, tb, tf, tb / tf, 100 * 2.0 * nq * n * d / (tb * 1e-3) / F16_PEAK, n * d * 2 / (tb * 1e-3), min(rb), max(rb),
                            min(rf), max(rf), same))
        if nq == 16:
            lines.append("# nq = 16: bytes/s of the rows against the HBM peak of %.0e: row-major and col-major above" % HBM_PEAK)
        tt = timed(lambda: torch_knn(x16, xq.half(), k, metric))
        lines.append("torch matmul + topk (half tensors, 1 Mi-row chunks), nq = %d: %.2f ms (min %.2f max %.2f)" % ((nq,) + tt))
        t_search = timed(lambda: f16.search_torch(xq, k, D=Df, I=If))[0]
        lines.append("copy-and-clone route, nq = %d: widen %.1f ms + add to Flat and clone with use_float16 %.1f ms + search %.2f ms = %.1f ms (wall, once)"
                     % (nq, t_widen, t_build, t_search, t_widen + t_build + t_search))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
