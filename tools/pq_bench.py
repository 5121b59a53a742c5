#!/usr/bin/env python3
"""PQ scan measurement (DESIGN.md "PQ"): PQ16 and PQ64 at d = 128 over synthetic clustered rows, k = 10.

  python3 tools/pq_bench.py [--rows 1000000,10000000] [--nq 1024,10000] [--M 16,64] [--out profiles/pq_scan.txt] [--no-pmc]

Per (N, M, nq): ms per search (HIP events around search_torch, inputs resident), (query, row, m) lookups per second set against the
conflict-free LDS gather rate of the table layout (scalar ds_read_b32: 32 pair-lookups per clock and CU; float2 / float4 via
ds_read_b64 / b128: 64), code bytes streamed per second (ceil(nq / query block) N M), and for context the exact Flat search on the
same rows with PQ's recall@10 against it.  SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE come from a counter-only rocprofv3 --pmc run of
this script's --pmc-child mode (a process of its own: counters are never collected together with any tracing)."""
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

D, K, CUS, CLOCK_HZ = 128, 10, 256, 2.4e9
GATHER_PER_CLK = {1: 32, 2: 64, 4: 64}  # pair-lookups per clock and CU by queries interleaved per table entry


def width(M):
    return 4 if M <= 32 else (2 if M <= 64 else 1)


def build(mf, torch, n, Ms, with_flat):
    """rows -> {M: PQ index}, Flat index | None; rows are generated on the device block by block"""
    blk = 1 << 20
    sample = mf.synth_clustered_torch(min(n, 200000), D, 7, 0).cpu().numpy()
    pqs = {}
    for M in Ms:
        ix = mf.index_factory(D, f"PQ{M}", mf.METRIC_L2)
        ix.train(sample)
        pqs[M] = ix
    flat = mf.index_factory(D, "Flat", mf.METRIC_L2) if with_flat else None
    for r0 in range(0, n, blk):
        x = mf.synth_clustered_torch(min(blk, n - r0), D, 7, r0)
        for ix in pqs.values():
            ix.add_torch(x)
        if flat is not None:
            flat.add_torch(x)
        torch.cuda.synchronize()
    return pqs, flat


def timed(torch, ix, xq, steps, warmup=1):
    out = None
    for _ in range(warmup):
        out = ix.search_torch(xq, K)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        out = ix.search_torch(xq, K)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps, out


def pmc_child(args):
    import torch

    import mi355_faiss as mf

    n, M, nq = args.rows[0], args.M[0], args.nq[0]
    pqs, _ = build(mf, torch, n, [M], False)
    xq = mf.synth_clustered_torch(nq, D, 99, 0)
    pqs[M].search_torch(xq, K)
    torch.cuda.synchronize()


def pmc_run(n, M, nq):
    """-> {counter: sum over the pq_scan_kernel dispatches} from a counter-only rocprofv3 run of the child mode"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--pmc", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "--output-format", "csv", "-d", tmp, "--",
               sys.executable, os.path.abspath(__file__), "--pmc-child", "--rows", str(n), "--M", str(M), "--nq", str(nq)]  # fmt: skip
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": (r.stderr or r.stdout)[-300:]}
        tot = {}
        for path in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "pq_scan_kernel" in row.get("Kernel_Name", ""):
                    tot[row["Counter_Name"]] = tot.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
        return tot


def main():
    ap = argparse.ArgumentParser()
    lst = lambda s: [int(v) for v in s.split(",")]
    ap.add_argument("--rows", type=lst, default=[1000000, 10000000])
    ap.add_argument("--nq", type=lst, default=[1024, 10000])
    ap.add_argument("--M", type=lst, default=[16, 64])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-pmc", action="store_true")
    ap.add_argument("--pmc-child", action="store_true")
    args = ap.parse_args()
    if args.pmc_child:
        return pmc_child(args)
    import torch

    import mi355_faiss as mf

    lines, records = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/pq_bench.py: d = {D}, k = {K}, L2, synthetic clustered rows (1024 centres, sigma 0.1); {torch.cuda.get_device_name(0)}")
    say("# model: conflict-free LDS gathers per clock and CU 32 (scalar) / 64 (float2, float4) x %d CUs x %.1f GHz" % (CUS, CLOCK_HZ / 1e9))
    for n in args.rows:
        pqs, flat = build(mf, torch, n, args.M, True)
        for nq in args.nq:
            xq = mf.synth_clustered_torch(nq, D, 99, 0)
            ms_flat, (_, I_flat) = timed(torch, flat, xq, args.steps)
            say(f"N={n} nq={nq} Flat (exact, context): {ms_flat:.2f} ms per search")
            for M, ix in pqs.items():
                ms, (_, I) = timed(torch, ix, xq, args.steps)
                Q = ix.get_stat("pq_query_block")
                launches, rescans = ix.get_stat("pq_scan_launches"), ix.get_stat("pq_scan_rescans")
                hits = (I.unsqueeze(2) == I_flat.unsqueeze(1)).any(dim=2).float().sum(dim=1).mean().item() / K
                lookups = nq * n * M / (ms * 1e-3)
                peak = GATHER_PER_CLK[width(M)] * CUS * CLOCK_HZ
                stream = -(-nq // Q) * n * M / (ms * 1e-3)
                rec = dict(N=n, nq=nq, M=M, ms=ms, query_block=Q, layout_width=width(M), lookups_per_s=lookups, lds_peak_fraction=lookups / peak,
                           code_bytes_per_s=stream, recall_at_10=hits, flat_ms=ms_flat, scan_launches=launches, rescans=rescans)  # fmt: skip
                records.append(rec)
                say(f"N={n} nq={nq} PQ{M}: {ms:.2f} ms per search; {lookups / 1e12:.3f} T lookups/s = {100 * lookups / peak:.1f} % of the "
                    f"conflict-free LDS rate of the { {1: 'scalar', 2: 'float2', 4: 'float4'}[width(M)] } layout; codes streamed {stream / 1e9:.1f} GB/s "
                    f"(query block {Q}); recall@10 vs Flat {hits:.3f}; {launches} scan launches, {rescans} rescans")  # fmt: skip
        del pqs, flat
        torch.cuda.empty_cache()
    if not args.no_pmc:
        n, nq = args.rows[0], args.nq[0]
        for M in args.M:
            c = pmc_run(n, M, nq)
            if "error" in c or not c:
                say(f"pmc N={n} nq={nq} PQ{M}: NOT TAKEN ({c.get('error', 'no pq_scan_kernel rows in the counter file')})")
                continue
            conf, act = c.get("SQ_LDS_BANK_CONFLICT", 0.0), c.get("SQ_LDS_IDX_ACTIVE", 0.0)
            say(f"pmc N={n} nq={nq} PQ{M} (build + one search, pq_scan_kernel dispatches only): SQ_LDS_BANK_CONFLICT {conf:.4g}, "
                f"SQ_LDS_IDX_ACTIVE {act:.4g}, conflict share {100 * conf / max(act, 1):.1f} %")
            records.append(dict(pmc=True, N=n, nq=nq, M=M, SQ_LDS_BANK_CONFLICT=conf, SQ_LDS_IDX_ACTIVE=act))
    say("json " + json.dumps(records))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
