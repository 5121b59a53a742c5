#!/usr/bin/env python3
"""PQ<M>x4fs against PQ<M>: the 4-bit scan on the int8 matrix pipe next to the 8-bit LDS-gather scan, same rows, same queries.

  python3 tools/pqfs_bench.py [--rows 10000000] [--nq 10000] [--M 32] [--repeats 5] [--out profiles/pqfs_scan.txt]

d = 128, k = 10, L2, synthetic clustered rows.  The two indexes are searched ALTERNATELY, --repeats times each after a warm-up of both
(HIP events around search_torch, inputs resident); reported per kind: median and min .. max of the step time, (query, row) pairs per
second, recall@10 against the exact Flat search of the same rows, and for the 4-bit kind the share of the int8 matrix peak its padded
GEMM reaches: 2 x 16 x 4 ceil(M / 4) operations per (query, row) over the step time, against 256 CUs x 4 SIMDs x 2.4 GHz x 2048
operations per clock (v_mfma_i32_16x16x64_i8 taken as 16 clocks).  The step time includes tables, selection and emission, so the share is an
end-to-end figure, not the scan kernel's."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))

D, K = 128, 10
I8_PEAK_OPS = 256 * 4 * 2.4e9 * 2048


def step_ms(torch, ix, xq):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = ix.search_torch(xq, K)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import mi355_faiss as mf

    if not torch.cuda.is_available():
        sys.exit("tools/pqfs_bench.py measures on the GPU: no device is visible")
    n, nq, M = args.rows, args.nq, args.M
    kinds = {f"PQ{M}": mf.index_factory(D, f"PQ{M}", mf.METRIC_L2), f"PQ{M}x4fs": mf.index_factory(D, f"PQ{M}x4fs", mf.METRIC_L2)}
    sample = mf.synth_clustered_torch(min(n, 200000), D, 7, 0).cpu().numpy()
    for ix in kinds.values():
        ix.train(sample)
    flat = mf.index_factory(D, "Flat", mf.METRIC_L2)
    for r0 in range(0, n, 1 << 20):
        x = mf.synth_clustered_torch(min(1 << 20, n - r0), D, 7, r0)
        for ix in list(kinds.values()) + [flat]:
            ix.add_torch(x)
        torch.cuda.synchronize()
    xq = mf.synth_clustered_torch(nq, D, 99, 0)
    _, I_flat = flat.search_torch(xq, K)
    times = {name: [] for name in kinds}
    recall = {}
    for rep in range(args.repeats + 1):  # (rep 0 warms both up)
        for name, ix in kinds.items():
            ms, (_, I) = step_ms(torch, ix, xq)
            if rep == 0:
                recall[name] = (I.unsqueeze(2) == I_flat.unsqueeze(1)).any(dim=2).float().sum(dim=1).mean().item() / K
            else:
                times[name].append(ms)
    lines, recs = [f"# tools/pqfs_bench.py: N = {n}, d = {D}, nq = {nq}, k = {K}, L2, {args.repeats} alternating repeats; {torch.cuda.get_device_name(0)}"], []
    for name, ix in kinds.items():
        t = times[name]
        med = statistics.median(t)
        rec = dict(kind=name, N=n, nq=nq, M=M, ms_median=med, ms_min=min(t), ms_max=max(t), pairs_per_s=nq * n / (med * 1e-3), recall_at_10=recall[name])
        line = f"{name}: {med:.1f} ms per search (min {min(t):.1f}, max {max(t):.1f}); {rec['pairs_per_s'] / 1e12:.3f} T pairs/s; recall@10 vs Flat {recall[name]:.3f}"
        if name.endswith("fs"):
            ops = 2.0 * 16 * 4 * -(-M // 4) * nq * n
            rec["int8_peak_share"] = ops / (med * 1e-3) / I8_PEAK_OPS
            rec["scan_launches"], rec["rescans"] = ix.get_stat("pqfs_scan_launches"), ix.get_stat("pqfs_scan_rescans")
            line += f"; {100 * rec['int8_peak_share']:.1f} % of the int8 matrix peak end to end; {rec['scan_launches']} scan launches a search, {rec['rescans']} rescans"
        lines.append(line)
        recs.append(rec)
    a, b = times[f"PQ{M}"], times[f"PQ{M}x4fs"]
    lines.append(f"ratio PQ{M} / PQ{M}x4fs step time: median {statistics.median(a) / statistics.median(b):.2f} (pairwise min {min(x / y for x, y in zip(a, b)):.2f}, max {max(x / y for x, y in zip(a, b)):.2f})")
    lines.append("json " + json.dumps(recs))
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
