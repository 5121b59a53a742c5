#!/usr/bin/env python3
"""IVFPQ scan measurement, k = 10, L2, synthetic clustered rows:

  python3 tools/ivfpq_bench.py [--configs 4096:16:128:10000000:10000:8+32,1024:96:768:1000000:10000:16] [--out profiles/ivfpq_scan.txt] [--no-pmc]

A configuration is nlist:M:d:N:nq:nprobe[+nprobe...].  The parent process never opens the GPU: every GPU step is a child process of
this script (--child) under its own time limit, the steps are chained and the first failure ends the run.  Per configuration and
nprobe the child reports ms per batch (HIP events around search_torch, inputs resident) and, from a second pass with the index's
kernel timing on, the share of ivfpq_scan_kernel in it; (query, probed row, m) lookups per second against the conflict-free LDS
gather rate of the table layout (3.93e13 float4 / float2, 1.97e13 scalar); code bytes per second; recall@10 against
the exact IVF<n>,Flat search with the same nprobe on the same rows.  SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE come from a counter-only
rocprofv3 --pmc run of the child (a process of its own: counters are never collected together with any tracing)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))

K = 10
GATHER_RATE = {1: 1.97e13, 2: 3.93e13, 4: 3.93e13}  # lookups/s by queries interleaved per table entry
DEFAULT = "4096:16:128:10000000:10000:8+32,1024:96:768:1000000:10000:16"


def width(M):
    return 4 if M <= 32 else (2 if M <= 64 else 1)


def parse(cfg):
    nlist, M, d, n, nq, nps = cfg.split(":")
    return int(nlist), int(M), int(d), int(n), int(nq), [int(v) for v in nps.split("+")]


def child(cfg, pmc_only):
    import torch

    import mi355_faiss as mf

    nlist, M, d, n, nq, nprobes = parse(cfg)
    blk = 1 << 20
    sample = mf.synth_clustered_torch(min(n, max(64 * nlist, 100000)), d, 7, 0).cpu().numpy()
    ix = mf.index_factory(d, f"IVF{nlist},PQ{M}", mf.METRIC_L2)
    ix.train(sample)
    flat = None
    if not pmc_only:
        flat = mf.index_factory(d, f"IVF{nlist},Flat", mf.METRIC_L2)
        flat.ivf_set_centroids(ix.ivf_centroids())
    for r0 in range(0, n, blk):
        x = mf.synth_clustered_torch(min(blk, n - r0), d, 7, r0)
        ix.add_torch(x)
        if flat is not None:
            flat.add_torch(x)
        torch.cuda.synchronize()
    xq = mf.synth_clustered_torch(nq, d, 99, 0)
    if pmc_only:
        ix.search_torch(xq, K, nprobe=nprobes[-1])
        torch.cuda.synchronize()
        return
    sizes = [ix.ivfpq_list_size(l) for l in range(nlist)]
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
        _, I_flat = flat.search_torch(xq, K, nprobe=nprobe)
        torch.cuda.synchronize()
        recall = (I.unsqueeze(2) == I_flat.unsqueeze(1)).any(dim=2).float().sum(dim=1).mean().item() / K
        rows = nq * nprobe * (n / nlist)  # probed rows, at the mean list size
        Q = ix.get_stat("ivfpq_pair_block")
        print("json " + json.dumps(dict(
            config=cfg, nprobe=nprobe, ms=ms, scan_ms=scan_ms, scan_launches_timed=launches_timed, other_ms=ms - scan_ms, pair_block=Q,
            layout_width=width(M), lookups_per_s=rows * M / (ms * 1e-3), lds_rate_fraction=rows * M / (ms * 1e-3) / GATHER_RATE[width(M)],
            code_bytes_per_s=rows * M / Q / (ms * 1e-3), recall_at_10_vs_ivfflat=recall, scan_launches=ix.get_stat("ivfpq_scan_launches"),
            rescans=ix.get_stat("ivfpq_scan_rescans"), largest_list=max(sizes), empty_lists=sum(1 for s in sizes if s == 0))), flush=True)


def run_child(cfg, limit, pmc):
    """-> (records, error | None) of one child process under its own time limit"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg]
    tmp = None
    if pmc:
        tmp = tempfile.mkdtemp(prefix="ivfpq_pmc_")
        cmd = ["rocprofv3", "--pmc", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "--output-format", "csv", "-d", tmp, "--"] + cmd + ["--pmc-only"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return [], f"time limit of {limit} s"
    if r.returncode != 0:
        return [], f"exit status {r.returncode}: {(r.stderr or r.stdout)[-400:]}"
    if not pmc:
        return [json.loads(line[5:]) for line in r.stdout.splitlines() if line.startswith("json ")], None
    tot = {}
    for path in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "ivfpq_scan_kernel" in row.get("Kernel_Name", ""):
                tot[row["Counter_Name"]] = tot.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    return [dict(pmc=True, config=cfg, **tot)], None if tot else "no ivfpq_scan_kernel rows in the counter file"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=DEFAULT)
    ap.add_argument("--limit", type=int, default=900, help="seconds one child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-pmc", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--pmc-only", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.pmc_only)
    lines, records = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/ivfpq_bench.py: k = {K}, L2, synthetic clustered rows (1024 centres, sigma 0.1), configurations nlist:M:d:N:nq:nprobes")
    say("# model: conflict-free LDS gathers 3.93e13 lookups/s (float4 / float2 layouts), 1.97e13 (scalar)")
    failed = None
    for pmc in ([False] if args.no_pmc else [False, True]):
        for cfg in args.configs.split(","):
            recs, err = run_child(cfg, args.limit, pmc)
            if err:
                say(f"{'pmc ' if pmc else ''}{cfg}: NOT TAKEN ({err})")
                failed = err
                break
            records += recs
            for r in recs:
                if pmc:
                    conf, act = r.get("SQ_LDS_BANK_CONFLICT", 0.0), r.get("SQ_LDS_IDX_ACTIVE", 0.0)
                    say(f"pmc {cfg} (train + add + one search, ivfpq_scan_kernel dispatches only): SQ_LDS_BANK_CONFLICT {conf:.4g}, "
                        f"SQ_LDS_IDX_ACTIVE {act:.4g}, conflict share {100 * conf / max(act, 1):.1f} %")
                else:
                    say(f"{cfg} nprobe={r['nprobe']}: {r['ms']:.2f} ms per batch (ivfpq_scan_kernel {r['scan_ms']:.2f} ms in {r['scan_launches_timed']} "
                        f"launches, coarse quantiser + grouping + selection + emit {r['other_ms']:.2f} ms); {r['lookups_per_s'] / 1e12:.3f} T lookups/s = "
                        f"{100 * r['lds_rate_fraction']:.1f} % of the conflict-free LDS rate; codes {r['code_bytes_per_s'] / 1e9:.1f} GB/s (pair block "
                        f"{r['pair_block']}); recall@10 vs IVF,Flat {r['recall_at_10_vs_ivfflat']:.3f}; {r['rescans']} rescans; largest list "
                        f"{r['largest_list']}, {r['empty_lists']} empty")
        if failed:  # a failed GPU step ends the run: nothing more is started on the device
            break
    say("json " + json.dumps(records))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
