#!/usr/bin/env python3
"""Range-search measurement: FlatL2, d = 128, N = 1 M synthetic uniform rows, nq = 10 000 and nq = 1.

  python3 tools/range_bench.py [--rows 1000000] [--d 128] [--nqs 10000,1] [--out profiles/range_search.txt]

The radius is the median 10th-neighbour distance of the batch (from search(k = 10) on the same index).  Per batch size the child reports
  - ms per range_search call (host clock around the call, which ends in a stream synchronisation; the result lands in host memory),
  - hits per query,
  - the scan kernel's time (HIP events of set_kernel_timing around the launch) and, where it is the MFMA kernel, its fraction of the
    f32 matrix peak (157 TF) on 2 nq N d flops; the remainder of the call is sort + lims + labels + the D2H copies + the query staging,
  - next to it, on the same index, search(k = 10) with option prefilter = 0: the exact f32 MFMA kernel doing the same contraction --
    the yardstick for the scan --, its call time and its kernel time.
The parent process never opens the GPU: the measurement is a child process (--child) under its own time limit."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))

F32_MATRIX_PEAK = 157e12


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def kernel_ms(ix, fn, reps):
    """mean HIP-event time of the dominant kernel over `reps` calls (several launches of one call are summed)"""
    ix.set_kernel_timing(True)
    _, t0 = ix.kernel_time_stats()
    for _ in range(reps):
        fn()
    _, t1 = ix.kernel_time_stats()
    ix.set_kernel_timing(False)
    return (t1 - t0) / reps


def child(rows, d, nqs):
    import numpy as np
    import torch

    import mi355_faiss as mf

    ix = mf.index_factory(d, "Flat", mf.METRIC_L2)
    blk = 1 << 18
    for r0 in range(0, rows, blk):
        ix.add_torch(mf.synth_uniform_torch(min(blk, rows - r0), d, 7, r0))
        torch.cuda.synchronize()
    ix.set_option("prefilter", 0)  # search on the exact f32 MFMA kernel (nq >= 20) / the per-pair kernels (nq < 20)
    for nq in nqs:
        xq = mf.synth_uniform_torch(nq, d, 99, 0).cpu().numpy()
        D10, _ = ix.search(xq, 10)
        radius = float(np.median(D10[:, 9]))
        reps = 5 if nq >= 1000 else 20
        lims, D, I = ix.range_search(xq, radius)
        range_name = ix.last_kernel_info()["name"]
        t_range = timed(lambda: ix.range_search(xq, radius), 2, reps)
        k_range = kernel_ms(ix, lambda: ix.range_search(xq, radius), reps)
        ix.search(xq, 10)
        search_name = ix.last_kernel_info()["name"]
        t_search = timed(lambda: ix.search(xq, 10), 2, reps)
        k_search = kernel_ms(ix, lambda: ix.search(xq, 10), reps)
        flops = 2.0 * nq * rows * d
        print("json " + json.dumps(dict(
            rows=rows, d=d, nq=nq, radius=radius, hits=int(lims[-1]), hits_per_query=float(lims[-1]) / nq, reps=reps,
            range_ms_median=statistics.median(t_range), range_ms_min=min(t_range), range_ms_max=max(t_range),
            range_kernel=range_name, range_kernel_ms=k_range, range_rest_ms=statistics.median(t_range) - k_range,
            range_kernel_peak_fraction=flops / (k_range * 1e-3) / F32_MATRIX_PEAK,
            range_rescans=ix.get_stat("range_rescans"),
            search_ms_median=statistics.median(t_search), search_ms_min=min(t_search), search_ms_max=max(t_search),
            search_kernel=search_name, search_kernel_ms=k_search, search_kernel_peak_fraction=flops / (k_search * 1e-3) / F32_MATRIX_PEAK)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nqs", default="10000,1")
    ap.add_argument("--limit", type=int, default=420, help="seconds the child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    nqs = [int(v) for v in args.nqs.split(",")]
    if args.child:
        return child(args.rows, args.d, nqs)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/range_bench.py: FlatL2 d = {args.d}, N = {args.rows} synthetic uniform rows; radius = the batch's median 10th-neighbour distance")
    say("# call times: host clock around the call (median of the repetitions after 2 warm-up calls; min .. max); kernel times: HIP events around the launch")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(args.rows), "--d", str(args.d), "--nqs", args.nqs]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        say(f"NOT TAKEN (time limit of {args.limit} s)")
        return 1
    if r.returncode != 0:
        say(f"NOT TAKEN (exit status {r.returncode}: {(r.stderr or r.stdout)[-400:]})")
        return 1
    recs = [json.loads(line[5:]) for line in r.stdout.splitlines() if line.startswith("json ")]
    for c in recs:
        say(f"nq = {c['nq']}: range_search {c['range_ms_median']:.2f} ms per call ({c['range_ms_min']:.2f} .. {c['range_ms_max']:.2f}, {c['reps']} calls), "
            f"{c['hits_per_query']:.1f} hits per query at radius {c['radius']:.4f}; scan {c['range_kernel']} {c['range_kernel_ms']:.2f} ms = "
            f"{100 * c['range_kernel_peak_fraction']:.1f} % of the f32 matrix peak, sort + lims + labels + copies + staging {c['range_rest_ms']:.2f} ms; "
            f"{c['range_rescans']} rescans so far")
        say(f"nq = {c['nq']}: search(k = 10, prefilter = 0) {c['search_ms_median']:.2f} ms per call ({c['search_ms_min']:.2f} .. {c['search_ms_max']:.2f}); "
            f"{c['search_kernel']} {c['search_kernel_ms']:.2f} ms = {100 * c['search_kernel_peak_fraction']:.1f} % of the f32 matrix peak")
    say("json " + json.dumps(recs))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
