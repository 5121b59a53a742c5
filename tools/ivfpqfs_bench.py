#!/usr/bin/env python3
"""IndexIVFPQFastScan against IVF<n>,PQ<M>: 4-bit lists on the int8 matrix pipe next to the 8-bit LDS-gather scan, with
and without ivfpq_precomputed_table; same rows, same queries, same request.

  python3 tools/ivfpqfs_bench.py [--rows 10000000] [--nq 10000] [--M 32] [--nlist 4096] [--nprobe 32] [--repeats 5] [--out profiles/ivfpqfs_scan.txt]

d = 128, k = 10, L2.  Data: x = z W, z uniform in [0, 1)^16, W a fixed 16 x 128 Gaussian matrix -- rows of intrinsic dimension 16, on which
IVF<n>,PQ<M> has a meaningful recall (the clustered set of tools/pqfs_bench.py does not).  The three routes are searched ALTERNATELY,
--repeats times each after a warm-up of all (HIP events around search_torch, inputs resident).  Reported per route: median and min .. max
of the step time, (query, row) pairs per second at the nominal nq nprobe N / nlist rows, recall@10 against the exact Flat search, and for
the 4-bit kind the share of the int8 matrix peak as tools/pqfs_bench.py defines it.  The step time includes the coarse search, the
tables, selection and emission: the share is an end-to-end figure, not the scan kernel's."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))

D, K, DZ = 128, 10, 16
I8_PEAK_OPS = 256 * 4 * 2.4e9 * 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000000)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import mi355_faiss as mf

    if not torch.cuda.is_available():
        sys.exit("tools/ivfpqfs_bench.py measures on the GPU: no device is visible")
    n, nq, M, nlist, nprobe = args.rows, args.nq, args.M, args.nlist, args.nprobe
    W = torch.randn((DZ, D), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda")

    def rows(count, seed, row0):
        return (mf.synth_uniform_torch(count, DZ, seed, row0) @ W).contiguous()

    pq = mf.index_factory(D, f"IVF{nlist},PQ{M}", mf.METRIC_L2)
    fs = mf.IndexIVFPQFastScan(D, nlist, M, 4, mf.METRIC_L2)
    flat = mf.index_factory(D, "Flat", mf.METRIC_L2)
    sample = rows(min(n, 400000), 7, 0).cpu().numpy()
    for ix in (pq, fs):
        ix.train(sample)
    for r0 in range(0, n, 1 << 20):
        x = rows(min(1 << 20, n - r0), 7, r0)
        for ix in (pq, fs, flat):
            ix.add_torch(x)
        torch.cuda.synchronize()
    xq = rows(nq, 99, 0)
    _, I_flat = flat.search_torch(xq, K)
    routes = [(f"IVF{nlist},PQ{M}", pq, 0), (f"IVF{nlist},PQ{M} precomputed", pq, 1), (f"IndexIVFPQFastScan M={M}", fs, None)]
    times, recall = {name: [] for name, _, _ in routes}, {}
    for rep in range(args.repeats + 1):  # (rep 0 warms every route up)
        for name, ix, opt in routes:
            if opt is not None:
                ix.set_option("ivfpq_precomputed_table", opt)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _, I = ix.search_torch(xq, K, nprobe=nprobe)
            b.record()
            torch.cuda.synchronize()
            if rep == 0:
                recall[name] = (I.unsqueeze(2) == I_flat.unsqueeze(1)).any(dim=2).float().sum(dim=1).mean().item() / K
            else:
                times[name].append(a.elapsed_time(b))
    pairs = nq * nprobe * n / nlist
    lines = [f"# tools/ivfpqfs_bench.py: N = {n}, d = {D}, M = {M}, nlist = {nlist}, nprobe = {nprobe}, nq = {nq}, k = {K}, L2, x = z W with z in [0, 1)^{DZ}; "
             f"{args.repeats} alternating repeats; {torch.cuda.get_device_name(0)}"]
    recs = []
    for name, ix, _ in routes:
        t = times[name]
        med = statistics.median(t)
        rec = dict(route=name, ms_median=med, ms_min=min(t), ms_max=max(t), pairs_per_s=pairs / (med * 1e-3), recall_at_10=recall[name])
        line = f"{name}: {med:.1f} ms per search (min {min(t):.1f}, max {max(t):.1f}); {rec['pairs_per_s'] / 1e9:.1f} G pairs/s; recall@10 vs Flat {recall[name]:.3f}"
        if ix is fs:
            rec["int8_peak_share"] = 2.0 * 16 * 4 * -(-M // 4) * pairs / (med * 1e-3) / I8_PEAK_OPS
            rec["scan_launches"], rec["rescans"] = ix.get_stat("ivfpqfs_scan_launches"), ix.get_stat("ivfpqfs_scan_rescans")
            line += f"; {100 * rec['int8_peak_share']:.2f} % of the int8 matrix peak end to end; {rec['scan_launches']} scan launches a search, {rec['rescans']} rescans"
        lines.append(line)
        recs.append(rec)
    lines.append("json " + json.dumps(recs))
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
