#!/usr/bin/env python3
"""HNSW<M> against HNSW<M>,SQ8 on the same rows, k = 10:

  python3 tools/hnsw_sq_bench.py [--d 768 --rows 1000000 --M 32 --efsearch 128 --data clustered --sigma 1.0 --normalize --metric L2]
                                 [--nq 10000 --repeats 5 --out profiles/hnsw_sq.txt]

The defaults are the shape and flags of README's `bench.py --index IDMap,HNSW32` line (same generators and seeds).  The parent process
never opens the GPU: the measurement is ONE child process of this script (--child) under its own time limit, which builds both kinds
(default concurrent build) and an exact Flat index from the same rows and then searches the two kinds ALTERNATELY.  Per kind it reports
ms per batch and QPS (HIP events around search_torch, inputs resident, the median of the repeats and their range), recall@10 against the
exact Flat index on the raw rows, hnsw_store_bytes, and the walk statistics of one more search with kernel timing on (distance
evaluations per query, rows fetched from each store, bytes one evaluation reads)."""
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

K = 10
DB_SEED, Q_SEED = 1234, 4321  # bench.py's


def child(a):
    import torch

    import mi355_faiss as mf

    metric = mf.METRIC_L2 if a.metric == "L2" else mf.METRIC_INNER_PRODUCT
    d, n, nq = a.d, a.rows, a.nq

    def gen(m, seed, row0=0):
        if a.data == "uniform":
            x = mf.synth_uniform_torch(m, d, seed, row0=row0)
        else:
            x = mf.synth_clustered_torch(m, d, seed, row0=row0, n_centers=a.centers, sigma=a.sigma)
        if a.normalize:
            x /= x.norm(dim=1, keepdim=True)
        return x

    kinds = [f"HNSW{a.M}", f"HNSW{a.M},SQ8"]
    ixs = {kd: mf.index_factory(d, kd, metric) for kd in kinds}
    exact = mf.index_factory(d, "Flat", metric)
    ixs[kinds[1]].train(gen(min(n, 1 << 18), DB_SEED).cpu().numpy())  # the range: the first 262 144 rows
    build_s = {kd: 0.0 for kd in kinds}
    slab = 1 << 16
    for s0 in range(0, n, slab):
        x = gen(min(slab, n - s0), DB_SEED, row0=s0)
        for kd in kinds:
            t0 = time.time()
            ixs[kd].add_torch(x)
            torch.cuda.synchronize()
            build_s[kd] += time.time() - t0
        exact.add_torch(x)
        torch.cuda.synchronize()
    xq = gen(nq, Q_SEED)
    _, I_exact = exact.search_torch(xq, K)
    torch.cuda.synchronize()
    res, ms = {}, {kd: [] for kd in kinds}
    for kd in kinds:  # warm-up: the dense level-0 copy and (f32 kind) the bf16 copy are made here
        _, res[kd] = ixs[kd].search_torch(xq, K, efSearch=a.efsearch)
        torch.cuda.synchronize()
    for _ in range(a.repeats):  # alternating
        for kd in kinds:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ixs[kd].search_torch(xq, K, efSearch=a.efsearch)
            e1.record()
            torch.cuda.synchronize()
            ms[kd].append(e0.elapsed_time(e1))
    for kd in kinds:
        ix = ixs[kd]
        ix.set_kernel_timing(True)
        ix.search_torch(xq, K, efSearch=a.efsearch)
        torch.cuda.synchronize()
        ws = ix.hnsw_walk_stats()
        ix.set_kernel_timing(False)
        recall = (res[kd].unsqueeze(2) == I_exact.unsqueeze(1)).any(dim=2).float().sum(dim=1).mean().item() / K
        med = statistics.median(ms[kd])
        print("json " + json.dumps(dict(
            kind=kd, ms=med, ms_min=min(ms[kd]), ms_max=max(ms[kd]), ms_all=[round(v, 3) for v in ms[kd]], qps=nq / (med * 1e-3), recall_at_10=recall,
            store_bytes=ix.get_stat("hnsw_store_bytes"), row_bytes=ix.get_stat("hnsw_row_bytes"), evaluations_per_query=ws["evaluations"] / nq,
            store_rows_per_query=ws["f32_rows"] / nq, bf16_rows_per_query=ws["bf16_rows"] / nq, build_seconds=build_s[kd],
            kernel=ix.last_kernel_info()["name"], grid=ix.last_kernel_info()["grid"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--efsearch", type=int, default=128)
    ap.add_argument("--data", choices=["uniform", "clustered"], default="clustered")
    ap.add_argument("--centers", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--normalize", action="store_true")
    ap.add_argument("--metric", choices=["L2", "IP"], default="L2")
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [v for v in sys.argv[1:] if v != "--child"]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/hnsw_sq_bench.py: d = {a.d}, N = {a.rows}, M = {a.M}, efSearch = {a.efsearch}, k = {K}, nq = {a.nq}, {a.metric}, {a.data} rows"
        + (f" ({a.centers} centres, sigma {a.sigma:g})" if a.data == "clustered" else "") + (", L2-normalised" if a.normalize else "")
        + f"; default concurrent build, efConstruction 40; {a.repeats} alternating repeats, median (min .. max)")
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        err = None if r.returncode == 0 else f"exit status {r.returncode}: {(r.stderr or r.stdout)[-600:]}"
    except subprocess.TimeoutExpired:
        r, err = None, f"time limit of {a.limit} s"
    recs = [] if r is None else [json.loads(line[5:]) for line in r.stdout.splitlines() if line.startswith("json ")]
    if err:
        say(f"NOT TAKEN ({err})")
    say("| kind | ms per batch | QPS | recall@10 vs Flat | hnsw_store_bytes | bytes per evaluation | evaluations per query | rows fetched per query (store / bf16 copy) | build s |")
    say("|---|---|---|---|---|---|---|---|---|")
    for x in recs:
        say(f"| {x['kind']} | {x['ms']:.2f} ({x['ms_min']:.2f} .. {x['ms_max']:.2f}) | {x['qps']:.0f} | {x['recall_at_10']:.4f} | {x['store_bytes']} | "
            f"{x['row_bytes']} | {x['evaluations_per_query']:.0f} | {x['store_rows_per_query']:.0f} / {x['bf16_rows_per_query']:.0f} | {x['build_seconds']:.1f} |")
    say("json " + json.dumps(recs))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if err else 0


if __name__ == "__main__":
    sys.exit(main())
