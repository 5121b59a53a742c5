#!/usr/bin/env python3
"""fp16 scalar-quantised inverted lists (GpuIndexIVFScalarQuantizer, QT_fp16) next to IVF<n>,SQ8 and IVF<n>,Flat on the
same rows, centroids and queries, k = 10, L2, synthetic clustered rows:

  python3 tools/sqfp16_bench.py [--config 4096:128:10000000:10000:32] [--out profiles/sqfp16_scan.txt]

The configuration is nlist:d:N:nq:nprobe.  The parent process never opens the GPU: the measurement is a child process of this script
(--child) under its own time limit.  Per kind the child reports ms per batch (HIP events around search_torch after a warm-up, inputs
resident), the device bytes of the index and recall@10 against the exact Flat search of the same rows; for the two coded kinds also,
from a second pass with the index's kernel timing on, the scan kernel's time and what it is of the least time the hardware could take
for the work the kernel reports (last_kernel_info's flops over the f16 matrix peak, its bytes over the HBM peak; for IVF<n>,SQ8 the
flops are vector-ALU work, so only the HBM share is given)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))

K = 10
PEAK_F16_MFMA_FLOPS = 2500.0e12  # v_mfma_f32_16x16x32_f16, dense
PEAK_HBM_BYTES = 8.0e12
DEFAULT = "4096:128:10000000:10000:32"


def child(cfg):
    import torch

    import mi355_faiss as mf

    nlist, d, n, nq, nprobe = (int(v) for v in cfg.split(":"))
    blk = 1 << 20
    sample = mf.synth_clustered_torch(min(n, max(64 * nlist, 100000)), d, 7, 0).cpu().numpy()
    sq8 = mf.index_factory(d, f"IVF{nlist},SQ8", mf.METRIC_L2)
    sq8.train(sample)  # the coarse centroids every kind below shares, and SQ8's range
    fp16 = mf.GpuIndexIVFScalarQuantizer(d, nlist, mf.QT_fp16, mf.METRIC_L2)
    flat = mf.index_factory(d, f"IVF{nlist},Flat", mf.METRIC_L2)
    exact = mf.index_factory(d, "Flat", mf.METRIC_L2)
    for ix in (fp16, flat):
        ix.ivf_set_centroids(sq8.ivf_centroids())
    for r0 in range(0, n, blk):
        x = mf.synth_clustered_torch(min(blk, n - r0), d, 7, r0)
        for ix in (fp16, sq8, flat, exact):
            ix.add_torch(x)
        torch.cuda.synchronize()
    xq = mf.synth_clustered_torch(nq, d, 99, 0)
    _, I_exact = exact.search_torch(xq, K)
    torch.cuda.synchronize()
    for name, ix in (("QT_fp16", fp16), (f"IVF{nlist},SQ8", sq8), (f"IVF{nlist},Flat", flat)):
        _, I = ix.search_torch(xq, K, nprobe=nprobe)  # warm-up: list views are built and code objects loaded here
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        steps = 5
        a.record()
        for _ in range(steps):
            ix.search_torch(xq, K, nprobe=nprobe)
        b.record()
        torch.cuda.synchronize()
        rec = dict(kind=name, config=cfg, ms=a.elapsed_time(b) / steps,
                   recall_at_10_vs_flat=(I.unsqueeze(2) == I_exact.unsqueeze(1)).any(dim=2).float().sum(dim=1).mean().item() / K)
        if ix is not flat:
            ix.set_kernel_timing(True)
            ix.search_torch(xq, K, nprobe=nprobe)
            torch.cuda.synchronize()
            launches, scan_ms = ix.kernel_time_stats()
            ix.set_kernel_timing(False)
            ki = ix.last_kernel_info()  # (of the last scan launch; the shares below are of the launches' summed work, so they are not taken from it)
            rows = nq * nprobe * (n / nlist)  # probed rows, at the mean list size
            dpad = (d + 31) // 32 * 32
            Q = ix.get_stat("sq_pair_block")
            flops = rows * dpad * 4.0 if ix is fp16 else 0.0
            nbytes = rows * (2 * d if ix is fp16 else d) / Q
            rec.update(scan_kernel=ki["name"], scan_ms=scan_ms, scan_launches_timed=launches, pair_block=Q, device_bytes=ix.get_stat("sq_device_bytes"),
                       f16_matrix_share=flops / PEAK_F16_MFMA_FLOPS / (scan_ms * 1e-3), hbm_share=nbytes / PEAK_HBM_BYTES / (scan_ms * 1e-3),
                       rescans=ix.get_stat("sq_scan_rescans"))
        else:
            rec.update(device_bytes=n * d * 4 + n * 8)  # f32 rows and ids: the lists' payload (the index's own statistic is not exported)
        print("json " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=DEFAULT)
    ap.add_argument("--limit", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    lines = [f"# tools/sqfp16_bench.py: k = {K}, L2, synthetic clustered rows (1024 centres, sigma 0.1), configuration nlist:d:N:nq:nprobe = {args.config}",
             f"# peaks: f16 matrix {PEAK_F16_MFMA_FLOPS:.3g} flop/s, HBM {PEAK_HBM_BYTES:.3g} B/s; flops = probed (query, row) pairs x padded d x 4 (hi and lo pass), "
             "bytes = probed rows x code bytes / pair block"]
    err = None
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", args.config], capture_output=True, text=True, timeout=args.limit)
        if r.returncode != 0:
            err = f"exit status {r.returncode}: {(r.stderr or r.stdout)[-400:]}"
    except subprocess.TimeoutExpired:
        r, err = None, f"time limit of {args.limit} s"
    records = [json.loads(line[5:]) for line in r.stdout.splitlines() if line.startswith("json ")] if r else []
    for c in records:
        s = f"{c['kind']}: {c['ms']:.2f} ms per batch; index {c['device_bytes'] / 1e9:.3f} GB; recall@10 vs exact Flat {c['recall_at_10_vs_flat']:.4f}"
        if "scan_ms" in c:
            s += (f"; {c['scan_kernel']} {c['scan_ms']:.2f} ms in {c['scan_launches_timed']} launches (pair block {c['pair_block']}, {c['rescans']} rescans): "
                  f"{100 * c['f16_matrix_share']:.1f} % of the f16 matrix peak, {100 * c['hbm_share']:.1f} % of HBM")
        lines.append(s)
    if err:
        lines.append(f"NOT TAKEN ({err})")
    lines.append("json " + json.dumps(records))
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if err else 0


if __name__ == "__main__":
    sys.exit(main())
