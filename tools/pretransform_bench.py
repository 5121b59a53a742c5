#!/usr/bin/env python3
"""Pre-transform apply and PCA training on one MI355X.  GPU box only; not part of the tests.

  python3 tools/pretransform_bench.py [--rows 4000000] [--shapes 768:64,768:128,768:256,128:64] [--reps 20] [--out profiles/pretransform.txt]

Per shape d_in -> d_out, on device-resident f32 rows: pretransform_apply_kernel through mvs_index_pretransform_apply_device (a matrix with a
bias, set by pretransform_set_linear), timed by device events after warm-up, the median of --reps calls.  Against each time:
  * the HBM time of reading x once and writing y once, n (d_in + d_out) 4 bytes, at the 6.3 TB/s a streaming kernel achieves and at the 8 TB/s
    of the data sheet (MI355X figures: HBM3E 8.0 TB/s spec, 6.29 TB/s measured);
  * the time of 2 n d_in d_out flop at the f32 matrix peak, 157.3 TFLOP/s (v_mfma_f32_32x32x2_f32: 64 flop per clock per SIMD);
  * torch.matmul + bias in f32 on the same tensors (torch.addmm), the outside yardstick: its order of summation is its own, so only its
    time is compared, and the largest difference of the two results is printed as a sanity figure.
Then PCA training at d_in = 768 -> 64 on n = 100 000 rows (host rows in, as mvs_index_train takes them), wall clock around a call that ends
synchronised, the median of three fresh indexes.
One JSON line per figure on stdout; --out also writes the table lines DESIGN.md quotes."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost")]

HBM_ACHIEVED, HBM_SPEC, F32_MATRIX_PEAK = 6.3e12, 8.0e12, 157.3e12


def timed_ms(fn, reps, warmup=3):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--shapes", default="768:64,768:128,768:256,128:64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train-rows", type=int, default=100_000)
    ap.add_argument("--train-d", type=int, default=768)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import mi355_faiss as mf

    if mf.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("no MI355X visible: this benchmark has no CPU fallback")
    lines = []

    def say(rec, text):
        print(json.dumps(rec), flush=True)
        lines.append(text)

    n = args.rows
    rng = np.random.default_rng(0)
    for shape in [v for v in args.shapes.split(",") if v]:
        di, do = (int(v) for v in shape.split(":"))
        ix = mf.index_factory(di, f"PCA{do},Flat", mf.METRIC_L2)
        A = (rng.standard_normal((do, di)) / np.sqrt(di)).astype(np.float32)
        b = rng.standard_normal(do).astype(np.float32)
        ix.pretransform_set_linear(0, A, b)
        x = torch.randn((n, di), dtype=torch.float32, device="cuda")
        y = torch.empty((n, do), dtype=torch.float32, device="cuda")
        At, bt = torch.from_numpy(A).cuda().t().contiguous(), torch.from_numpy(b).cuda()
        y2 = torch.empty_like(y)
        ms, lo, hi = timed_ms(lambda: ix.pretransform_apply_torch(x, y), args.reps)
        tms, tlo, thi = timed_ms(lambda: torch.addmm(bt, x, At, out=y2), args.reps)
        diff = float((y[:65536] - y2[:65536]).abs().max())
        nbytes, flop = n * (di + do) * 4.0, 2.0 * n * di * do
        hbm_ms, hbm_spec_ms, mat_ms = nbytes / HBM_ACHIEVED * 1e3, nbytes / HBM_SPEC * 1e3, flop / F32_MATRIX_PEAK * 1e3
        bound = "HBM" if hbm_ms >= mat_ms else "the f32 matrix pipe"
        rec = dict(what="apply", d_in=di, d_out=do, rows=n, ms=ms, ms_min=lo, ms_max=hi, bytes=nbytes, flop=flop, achieved_TBps=nbytes / ms / 1e9,
                   achieved_TFLOPs=flop / ms / 1e9, hbm_ms_at_6_3=hbm_ms, hbm_ms_at_8=hbm_spec_ms, matrix_peak_ms=mat_ms, bound=bound,
                   share_of_bound=max(hbm_ms, mat_ms) / ms, torch_addmm_ms=tms, torch_ms_min=tlo, torch_ms_max=thi, ratio_to_torch=ms / tms,
                   max_abs_diff_to_torch=diff)
        say(rec, f"apply {di} -> {do}, n = {n}: {ms:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {nbytes / ms / 1e9:.2f} TB/s of x + y, {flop / ms / 1e9:.1f} TFLOP/s; "
                 f"HBM time {hbm_ms:.3f} ms at 6.3 TB/s ({hbm_spec_ms:.3f} at 8), matrix-peak time {mat_ms:.3f} ms: bound by {bound}, "
                 f"{100 * max(hbm_ms, mat_ms) / ms:.0f} % of it; torch.addmm {tms:.3f} ms (x {ms / tms:.2f}); max |difference| {diff:.2e}")
        del x, y, y2, ix
        torch.cuda.empty_cache()
    # PCA training
    d, nt = args.train_d, args.train_rows
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))  # (a dense covariance: spectrum 1 / (1 + i) along a random orthonormal basis)
    xt = ((rng.standard_normal((nt, d)) * (1.0 / np.sqrt(1.0 + np.arange(d)))[None, :]) @ Q.T).astype(np.float32)
    secs = []
    for _ in range(3):
        ix = mf.index_factory(d, "PCA64,Flat", mf.METRIC_L2)
        t0 = time.perf_counter()
        ix.train(xt)  # (returns with the matrices on the host: synchronised)
        secs.append(time.perf_counter() - t0)
        assert ix.is_trained
    A64 = ix.pretransform_get_linear(0)[0].astype(np.float64)
    ortho = float(np.abs(A64 @ A64.T - np.eye(64)).max())
    ev = ix.pretransform_get_pca(0)[1]
    say(dict(what="pca_train", d_in=d, d_out=64, rows=nt, seconds=statistics.median(secs), seconds_all=secs, max_abs_AAt_minus_I=ortho,
             eigenvalues_head=[float(v) for v in ev[:4]]),
        f"PCA training {d} -> 64 on n = {nt} host rows: {statistics.median(secs):.3f} s (three fresh indexes: {', '.join('%.3f' % s for s in secs)}); "
        f"max |A A^T - I| = {ortho:.2e}, leading eigenvalues {', '.join('%.4f' % v for v in ev[:4])}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/pretransform_bench.py: device-resident f32 rows, device events, median after warm-up; one MI355X\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
