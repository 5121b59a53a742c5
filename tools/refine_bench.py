#!/usr/bin/env python3
"""<base>,RFlat measurement, k = 10, L2, synthetic clustered rows:

  python3 tools/refine_bench.py [--configs IVF4096,PQ32:128:10000000:10000:32;IVF4096,SQ8:128:10000000:10000:32]
                                [--k-factors 1,4,16,64] [--out profiles/refine.txt]

A configuration is base:d:N:nq:nprobe.  The parent process never opens the GPU: every GPU step is a child process of this script
(--child) under its own time limit, the steps are chained and the first failure ends the run.  Per configuration the child builds ONE
"<base>,RFlat" index and a Flat index on the same rows; the bare base is the refine index's own base (mvs_index_refine_base: the same
codes, searched directly), the true neighbours are the Flat index's.  It reports recall@10 and ms per batch of the bare base, and per
k_factor recall@10, ms per batch (HIP events around search_torch, inputs resident) and, from a second pass with the index's kernel timing
on, the time of refine_flat_kernel alone with its achieved bytes/s -- candidate rows fetched once, whole: nq * kb * 4 * dp bytes -- against
the measured random-row gather rate of the MI355X, 5.5 TB/s chip-wide."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))

K = 10
GATHER_BYTES_PER_S = 5.5e12  # random whole rows of a buffer far larger than the Infinity Cache, enough rows in flight
DEFAULT = "IVF4096,PQ32:128:10000000:10000:32;IVF4096,SQ8:128:10000000:10000:32"


def parse(cfg):
    base, d, n, nq, nprobe = cfg.split(":")
    return base, int(d), int(n), int(nq), int(nprobe)


def child(cfg, k_factors):
    import torch

    import mi355_faiss as mf

    base, d, n, nq, nprobe = parse(cfg)
    nlist = int(base[3 : base.index(",")]) if base.startswith("IVF") else 0
    blk = 1 << 20
    sample = mf.synth_clustered_torch(min(n, max(64 * nlist, 100000)), d, 7, 0).cpu().numpy()
    ix = mf.index_factory(d, base + ",RFlat", mf.METRIC_L2)
    ix.train(sample)
    flat = mf.index_factory(d, "Flat", mf.METRIC_L2)
    for r0 in range(0, n, blk):
        x = mf.synth_clustered_torch(min(blk, n - r0), d, 7, r0)
        ix.add_torch(x)
        flat.add_torch(x)
        torch.cuda.synchronize()
    xq = mf.synth_clustered_torch(nq, d, 99, 0)
    _, I_true = flat.search_torch(xq, K)
    torch.cuda.synchronize()

    def recall(I):
        return (I.unsqueeze(2) == I_true.unsqueeze(1)).any(dim=2).float().sum(dim=1).mean().item() / K

    def timed(index, steps=3):
        _, I = index.search_torch(xq, K, nprobe=nprobe)  # warm-up: the base's list view is built here
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            index.search_torch(xq, K, nprobe=nprobe)
        b.record()
        torch.cuda.synchronize()
        return I, a.elapsed_time(b) / steps

    I, ms = timed(ix.refine_base)
    print("json " + json.dumps(dict(config=cfg, k_factor=None, recall_at_10=recall(I), ms=ms, ms_per_10k=ms * 10000.0 / nq)), flush=True)
    for kf in k_factors:
        ix.k_factor = kf
        I, ms = timed(ix)
        before = ix.kernel_time_stats()
        ix.set_kernel_timing(True)
        ix.search_torch(xq, K, nprobe=nprobe)
        torch.cuda.synchronize()
        after = ix.kernel_time_stats()
        ix.set_kernel_timing(False)
        launches, refine_ms = after[0] - before[0], after[1] - before[1]
        ki = ix.last_kernel_info()
        chunk = ix.get_stat("refine_query_chunk")
        nbytes = ki["bytes"] * nq / min(nq, chunk) if launches > 1 else ki["bytes"]  # (the info describes the last pass)
        rate = nbytes / (max(refine_ms, 1e-9) * 1e-3)
        print("json " + json.dumps(dict(
            config=cfg, k_factor=kf, kb=ix.get_stat("refine_candidates"), recall_at_10=recall(I), ms=ms, ms_per_10k=ms * 10000.0 / nq,
            refine_ms=refine_ms, refine_launches=launches, refine_bytes=nbytes, refine_bytes_per_s=rate, gather_rate_share=rate / GATHER_BYTES_PER_S,
            lds_bytes=ki["lds_bytes"], query_chunk=chunk, store_bytes=ix.get_stat("refine_store_bytes"))), flush=True)


def run_child(cfg, k_factors, limit):
    """-> (records, error | None) of one child process under its own time limit"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--k-factors", k_factors]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return [], f"time limit of {limit} s"
    if r.returncode != 0:
        return [], f"exit status {r.returncode}: {(r.stderr or r.stdout)[-400:]}"
    return [json.loads(line[5:]) for line in r.stdout.splitlines() if line.startswith("json ")], None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=DEFAULT, help="base:d:N:nq:nprobe, separated by ';' (a base holds commas)")
    ap.add_argument("--k-factors", default="1,4,16,64")
    ap.add_argument("--limit", type=int, default=900, help="seconds one child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, [float(v) for v in args.k_factors.split(",")])
    lines, records = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/refine_bench.py: k = {K}, L2, synthetic clustered rows (1024 centres, sigma 0.1), configurations base:d:N:nq:nprobe; true "
        "neighbours from Flat on the same rows; the bare base is the refine index's own base index")
    say(f"# yardstick: refine_flat_kernel's nq * kb * 4 * dp bytes against {GATHER_BYTES_PER_S / 1e12:.1f} TB/s, the measured chip-wide rate of random whole rows")
    failed = None
    for cfg in args.configs.split(";"):
        recs, err = run_child(cfg, args.k_factors, args.limit)
        if err:
            say(f"{cfg}: NOT TAKEN ({err})")
            failed = err
            break  # a failed GPU step ends the run: nothing more is started on the device
        records += recs
        for r in recs:
            if r["k_factor"] is None:
                say(f"{cfg} bare base: recall@10 {r['recall_at_10']:.3f}, {r['ms_per_10k']:.2f} ms per 10 k queries")
                continue
            say(f"{cfg} RFlat k_factor={r['k_factor']:g} (kb {r['kb']}): recall@10 {r['recall_at_10']:.3f}, {r['ms_per_10k']:.2f} ms per 10 k queries; "
                f"refine_flat_kernel {r['refine_ms']:.3f} ms in {r['refine_launches']} launch(es) for {r['refine_bytes'] / 1e9:.3f} GB = "
                f"{r['refine_bytes_per_s'] / 1e12:.2f} TB/s = {100 * r['gather_rate_share']:.0f} % of the gather rate ({r['lds_bytes']} B of LDS per workgroup)")
    say("json " + json.dumps(records))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
