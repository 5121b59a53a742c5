#!/usr/bin/env python3
"""merge_from measurement: two halves of N = 10 M synthetic uniform rows, d = 128, merged on the device -- Flat,
IVF4096,Flat and IVF4096,PQ16.

  python3 tools/merge_bench.py [--rows 10000000] [--d 128] [--kinds 'Flat;IVF4096,Flat;IVF4096,PQ16'] [--out profiles/merge_bench.txt] [--profile]

Per kind the child reports
  - ms of A.merge_from(B) with a device synchronisation behind it (host clock; one call per freshly filled pair -- a merge cannot be
    repeated on the same rows), and of the first search afterwards, which derives the list views again,
  - what a user has to do without merge_from: reconstruct_n of B to the host, then add / add_with_ids into A, synchronised; for the
    coded kind the original rows are added again from host memory (reconstruct would give decoded rows, not the same codes),
  - the bytes the move must carry (B's rows read once and written once) over the device copy rate measured in the same process
    (a device-to-device copy of 1 GiB, read + written bytes per second), and the call's share of that bound.
--profile sets MVS_MERGE_PROFILE=1 in the child: the call's phases (growth allocation, move kernel, directory append, the source's reset)
on stderr, copied into the report.  IVF centroids are 4096 of the rows, the PQ codebooks random (no k-means: training is not part of either
side).  The parent process never opens the GPU: the measurement is a child process (--child) under its own time limit."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))


def child(rows, d, kinds):
    import numpy as np
    import torch

    import mi355_faiss as mf

    blk = 1 << 18
    host = np.empty((rows, d), dtype=np.float32)
    for r0 in range(0, rows, blk):
        host[r0 : r0 + blk] = mf.synth_uniform_torch(min(blk, rows - r0), d, 7, r0).cpu().numpy()
    half = rows // 2
    rng = np.random.default_rng(11)

    # the device copy rate of this box: read + written bytes per second of a 1 GiB device-to-device copy
    a, b = (torch.empty(1 << 30, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    a.copy_(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        a.copy_(b)
    torch.cuda.synchronize()
    copy_rate = 10 * 2.0 * (1 << 30) / (time.perf_counter() - t0)
    del a, b
    print("json " + json.dumps(dict(copy_rate=copy_rate)), flush=True)

    def make(kind):
        ix = mf.index_factory(d, kind, mf.METRIC_L2)
        if kind.startswith("IVF"):
            ix.ivf_set_centroids(host[:: rows // ix.nlist][: ix.nlist])
        if "PQ" in kind:
            M = ix.pq_info()[0]
            ix.pq_set_centroids(np.random.default_rng(3).standard_normal((M, 256, d // M)).astype(np.float32) * 0.3)
        return ix

    def fill(ix, x):
        step = 1 << 20
        for r0 in range(0, x.shape[0], step):
            ix.add(x[r0 : r0 + step])

    xq = host[rng.integers(0, rows, 32)]
    for kind in kinds:
        ivf = kind.startswith("IVF")
        add_id = half if ivf else 0  # (B numbers its rows from 0: an IVF kind stores the ids)
        A, B = make(kind), make(kind)
        fill(A, host[:half]), fill(B, host[half:])
        A.search(xq, 10, nprobe=8), B.search(xq, 10, nprobe=8)  # (the list views exist, as on indexes in use)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        A.merge_from(B, add_id)
        torch.cuda.synchronize()
        t_merge = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        D1, I1 = A.search(xq, 10, nprobe=8)
        t_first = (time.perf_counter() - t0) * 1e3
        assert A.ntotal == rows and B.ntotal == 0
        del A, B
        A, B = make(kind), make(kind)
        fill(A, host[:half]), fill(B, host[half:])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        coded = "PQ" in kind or "SQ" in kind
        x = host[half:] if coded else B.reconstruct_n(0, rows - half)
        t_down = (time.perf_counter() - t0) * 1e3
        if ivf:
            step = 1 << 20
            for r0 in range(0, x.shape[0], step):
                A.add_with_ids(x[r0 : r0 + step], np.arange(r0, min(r0 + step, x.shape[0]), dtype=np.int64) + add_id)
        else:
            fill(A, x)
        torch.cuda.synchronize()
        t_host = (time.perf_counter() - t0) * 1e3
        D2, I2 = A.search(xq, 10, nprobe=8)
        same = bool(np.array_equal(D1.view(np.uint32), D2.view(np.uint32)) and np.array_equal(I1, I2))
        del A, B, x
        row_bytes = {"Flat": d * 4 + 4}.get(kind, 16 * ((int(kind.split("PQ")[1]) + 15) // 16) if "PQ" in kind else d * 4)  # (d a multiple of 32: no padding)
        moved = 2.0 * (rows - half) * row_bytes
        print("json " + json.dumps(dict(kind=kind, rows=rows, d=d, merge_ms=t_merge, first_search_ms=t_first, host_route_ms=t_host, host_download_ms=t_down,
                                        host_route="add again from host memory" if coded else "reconstruct_n + add", bytes_moved=moved,
                                        bound_ms=moved / copy_rate * 1e3, share_of_bound=(moved / copy_rate * 1e3) / t_merge, same_answers=same)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--kinds", default="Flat;IVF4096,Flat;IVF4096,PQ16", help="index strings separated by ';'")
    ap.add_argument("--limit", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="MVS_MERGE_PROFILE=1 in the child: the call's phases on stderr, copied here")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    kinds = args.kinds.split(";")
    if args.child:
        return child(args.rows, args.d, kinds)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/merge_bench.py: d = {args.d}, two halves of N = {args.rows} synthetic uniform rows, L2")
    say("# merge: A.merge_from(B) + device synchronisation (one call per freshly filled pair); host route: reconstruct_n of B + add into A (coded kinds: the original")
    say("# rows added again from host memory); bound: B's rows read once and written once at the device copy rate measured in the same process")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(args.rows), "--d", str(args.d), "--kinds", args.kinds]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, env=dict(os.environ, MVS_MERGE_PROFILE="1") if args.profile else None)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        for line in out.splitlines():
            if line.startswith("json "):
                say(line)
        say(f"NOT COMPLETE (time limit of {args.limit} s)")
        return 1
    if r.returncode != 0:
        say(f"NOT TAKEN (exit status {r.returncode}: {(r.stderr or r.stdout)[-600:]})")
        return 1
    recs = [json.loads(line[5:]) for line in r.stdout.splitlines() if line.startswith("json ")]
    for line in r.stderr.splitlines():
        if line.startswith("mergeprofile"):
            say("# " + line)
    for c in recs:
        if "copy_rate" in c:
            say(f"device copy rate (1 GiB device to device, read + written): {c['copy_rate'] / 1e12:.2f} TB/s")
            continue
        say(f"{c['kind']}: merge_from {c['merge_ms']:.1f} ms; host route ({c['host_route']}) {c['host_route_ms']:.1f} ms, of which the download {c['host_download_ms']:.1f} ms "
            f"({c['host_route_ms'] / c['merge_ms']:.1f} x); bound {c['bound_ms']:.2f} ms for {c['bytes_moved'] / 1e9:.2f} GB = {100 * c['share_of_bound']:.1f} % of the call; "
            f"first search afterwards {c['first_search_ms']:.1f} ms; answers equal to the host route's index: {c['same_answers']}")
    say("json " + json.dumps(recs))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
