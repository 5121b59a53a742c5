#!/usr/bin/env python3
"""SQ8 / IVF<n>,SQ8 scan measurement, k = 10, L2, synthetic clustered rows:

  python3 tools/sq_bench.py [--configs 4096:128:10000000:10000:8+32,0:768:1000000:10000:0] [--out profiles/sq_scan.txt]

A configuration is nlist:d:N:nq:nprobe[+nprobe...]; nlist = 0 is the bare SQ8 index (its nprobe is ignored).  The parent process never
opens the GPU: every GPU step is a child process of this script (--child) under its own time limit, the steps are chained and the
first failure ends the run.  Per configuration and nprobe the child reports ms per batch (HIP events around search_torch, inputs
resident) and, from a second pass with the index's kernel timing on, the share of sq8_scan_kernel in it; (query, probed row,
component) triples per second against the packed-f32 VALU model of DESIGN.md 3.9; the device bytes of the index next to those of the
f32 index on the same rows; recall@10 against the exact IVF<n>,Flat search with the same nprobe (SQ8: against Flat) on the same rows."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))

K = 10
# L2: one subtraction and one fma per (pair, row, component), two pairs per packed instruction -> 1 lane-instruction per triple;
# 256 CUs x 4 SIMDs x 16 lanes x 2.4e9 /s
VALU_LANE_OPS = 256 * 4 * 16 * 2.4e9
DEFAULT = "4096:128:10000000:10000:8+32,0:768:1000000:10000:0"


def parse(cfg):
    nlist, d, n, nq, nps = cfg.split(":")
    return int(nlist), int(d), int(n), int(nq), [int(v) for v in nps.split("+")]


def child(cfg):
    import torch

    import mi355_faiss as mf

    nlist, d, n, nq, nprobes = parse(cfg)
    blk = 1 << 20
    sample = mf.synth_clustered_torch(min(n, max(64 * nlist, 100000)), d, 7, 0).cpu().numpy()
    desc = f"IVF{nlist},SQ8" if nlist else "SQ8"
    ix = mf.index_factory(d, desc, mf.METRIC_L2)
    ix.train(sample)
    exact = mf.index_factory(d, f"IVF{nlist},Flat" if nlist else "Flat", mf.METRIC_L2)
    if nlist:
        exact.ivf_set_centroids(ix.ivf_centroids())
    for r0 in range(0, n, blk):
        x = mf.synth_clustered_torch(min(blk, n - r0), d, 7, r0)
        ix.add_torch(x)
        exact.add_torch(x)
        torch.cuda.synchronize()
    xq = mf.synth_clustered_torch(nq, d, 99, 0)
    sizes = [ix.ivfsq_list_size(l) for l in range(nlist)] if nlist else [n]
    for nprobe in nprobes:
        _, I = ix.search_torch(xq, K, nprobe=nprobe)  # warm-up: the list view is built here
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        steps = 3
        a.record()
        for _ in range(steps):
            ix.search_torch(xq, K, nprobe=nprobe)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / steps
        ix.set_kernel_timing(True)
        ix.search_torch(xq, K, nprobe=nprobe)
        torch.cuda.synchronize()
        launches_timed, scan_ms = ix.kernel_time_stats()
        ix.set_kernel_timing(False)
        _, I_exact = exact.search_torch(xq, K, nprobe=nprobe)
        torch.cuda.synchronize()
        recall = (I.unsqueeze(2) == I_exact.unsqueeze(1)).any(dim=2).float().sum(dim=1).mean().item() / K
        rows = nq * (nprobe * (n / nlist) if nlist else n)  # probed rows, at the mean list size
        print("json " + json.dumps(dict(
            config=cfg, nprobe=nprobe, ms=ms, scan_ms=scan_ms, scan_launches_timed=launches_timed, other_ms=ms - scan_ms,
            pair_block=ix.get_stat("sq_pair_block"), triples_per_s=rows * d / (ms * 1e-3), scan_triples_per_s=rows * d / (max(scan_ms, 1e-9) * 1e-3),
            valu_model_fraction=rows * d / (max(scan_ms, 1e-9) * 1e-3) / VALU_LANE_OPS, device_bytes=ix.get_stat("sq_device_bytes"),
            f32_row_bytes=n * d * 4, recall_at_10_vs_exact=recall, scan_launches=ix.get_stat("sq_scan_launches"),
            rescans=ix.get_stat("sq_scan_rescans"), largest_list=max(sizes), empty_lists=sum(1 for s in sizes if s == 0))), flush=True)


def run_child(cfg, limit):
    """-> (records, error | None) of one child process under its own time limit"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return [], f"time limit of {limit} s"
    if r.returncode != 0:
        return [], f"exit status {r.returncode}: {(r.stderr or r.stdout)[-400:]}"
    return [json.loads(line[5:]) for line in r.stdout.splitlines() if line.startswith("json ")], None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=DEFAULT)
    ap.add_argument("--limit", type=int, default=900, help="seconds one child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    lines, records = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/sq_bench.py: k = {K}, L2, synthetic clustered rows (1024 centres, sigma 0.1), configurations nlist:d:N:nq:nprobes (nlist 0: SQ8)")
    say(f"# model: one packed-f32 lane-instruction per (query, probed row, component) triple under L2, {VALU_LANE_OPS:.3g} lane-instructions/s")
    failed = None
    for cfg in args.configs.split(","):
        recs, err = run_child(cfg, args.limit)
        if err:
            say(f"{cfg}: NOT TAKEN ({err})")
            failed = err
            break  # a failed GPU step ends the run: nothing more is started on the device
        records += recs
        for r in recs:
            say(f"{cfg} nprobe={r['nprobe']}: {r['ms']:.2f} ms per batch (sq8_scan_kernel {r['scan_ms']:.2f} ms in {r['scan_launches_timed']} launches, "
                f"coarse quantiser + grouping + selection + emit {r['other_ms']:.2f} ms); scan {r['scan_triples_per_s'] / 1e12:.3f} T triples/s = "
                f"{100 * r['valu_model_fraction']:.1f} % of the packed-f32 model (pair block {r['pair_block']}); index {r['device_bytes'] / 1e9:.3f} GB on the "
                f"device against {r['f32_row_bytes'] / 1e9:.3f} GB of f32 rows; recall@10 vs the exact index {r['recall_at_10_vs_exact']:.3f}; "
                f"{r['rescans']} rescans of {r['scan_launches']} launches; largest list {r['largest_list']}, {r['empty_lists']} empty")
    say("json " + json.dumps(records))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
