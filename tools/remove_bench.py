#!/usr/bin/env python3
"""remove_ids measurement: Flat d = 128 and IVF4096,Flat at N = 10 M synthetic uniform rows, removing 1 %, 10 % and 50 %.

  python3 tools/remove_bench.py [--rows 10000000] [--d 128] [--kinds 'Flat;IVF4096,Flat'] [--fractions 0.01,0.1,0.5] [--out profiles/remove_ids.txt]

Per kind and fraction the child reports
  - ms of the remove_ids call with a device synchronisation behind it (host clock; one call per freshly filled index -- a removal cannot be
    repeated on the same rows),
  - what a user has to do without remove_ids: a fresh index plus add() of the surviving rows from host memory, synchronised (for IVF the
    centroids are set, not trained again: training is not part of either side),
  - the bytes the compaction must move (survivors read once and written once: rows, norms) over the 6.3 TB/s copy rate of the device,
    and the call's share of that bound.
The rows are a random member set (seeded) passed as an IDSelectorBatch.  IVF centroids are 4096 of the rows (no k-means: list balance is
that of uniform data).  The parent process never opens the GPU: the measurement is a child process (--child) under its own time limit."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))

COPY_RATE = 6.3e12  # bytes / s, the measured device copy rate


def child(rows, d, kinds, fractions):
    import numpy as np
    import torch

    import mi355_faiss as mf

    blk = 1 << 18
    host = np.empty((rows, d), dtype=np.float32)
    for r0 in range(0, rows, blk):
        host[r0 : r0 + blk] = mf.synth_uniform_torch(min(blk, rows - r0), d, 7, r0).cpu().numpy()
    rng = np.random.default_rng(11)

    def make(kind):
        ix = mf.index_factory(d, kind, mf.METRIC_L2)
        if kind.startswith("IVF"):
            ix.ivf_set_centroids(host[:: rows // ix.nlist][: ix.nlist])
        return ix

    def fill(ix, x):
        step = 1 << 20
        for r0 in range(0, x.shape[0], step):
            ix.add(x[r0 : r0 + step])

    for kind in kinds:
        for frac in fractions:
            gone = np.sort(rng.choice(rows, size=int(rows * frac), replace=False)).astype(np.int64)
            ix = make(kind)
            fill(ix, host)
            ix.search(host[:32], 10, nprobe=8)  # (the list views exist, as on an index in use)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            removed = ix.remove_ids(("batch", gone))
            torch.cuda.synchronize()
            t_remove = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            D1, I1 = ix.search(host[:32], 10, nprobe=8)  # the first search afterwards rebuilds what is derived (IVF: the list view)
            t_first = (time.perf_counter() - t0) * 1e3
            del ix
            keep = np.ones(rows, dtype=bool)
            keep[gone] = False
            surv = host[keep]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fresh = make(kind)
            fill(fresh, surv)
            torch.cuda.synchronize()
            t_rebuild = (time.perf_counter() - t0) * 1e3
            D2, I2 = fresh.search(host[:32], 10, nprobe=8)
            same = bool(np.array_equal(D1.view(np.uint32), D2.view(np.uint32)))
            row_bytes = d * 4 + (0 if kind.startswith("IVF") else 4)  # (d a multiple of 32: no padding; Flat carries a norm per row)
            moved = 2.0 * surv.shape[0] * row_bytes
            del fresh, surv
            print("json " + json.dumps(dict(kind=kind, rows=rows, d=d, fraction=frac, removed=int(removed), remove_ms=t_remove, first_search_ms=t_first,
                                            rebuild_ms=t_rebuild, bytes_moved=moved, bound_ms=moved / COPY_RATE * 1e3,
                                            share_of_bound=(moved / COPY_RATE * 1e3) / t_remove, same_distances=same)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--kinds", default="Flat;IVF4096,Flat", help="index strings separated by ';'")
    ap.add_argument("--fractions", default="0.01,0.1,0.5")
    ap.add_argument("--limit", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="MVS_REMOVE_PROFILE=1 in the child: the call's phases on stderr, copied here")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    kinds = args.kinds.split(";")
    fractions = [float(v) for v in args.fractions.split(",")]
    if args.child:
        return child(args.rows, args.d, kinds, fractions)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/remove_bench.py: d = {args.d}, N = {args.rows} synthetic uniform rows, L2; a random member set as an IDSelectorBatch")
    say("# remove: the remove_ids call + device synchronisation (one call per freshly filled index); rebuild: a fresh index + add() of the survivors from host memory;")
    say("# bound: survivors read once and written once (rows + norms) at 6.3 TB/s")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(args.rows), "--d", str(args.d), "--kinds", args.kinds, "--fractions", args.fractions]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, env=dict(os.environ, MVS_REMOVE_PROFILE="1") if args.profile else None)
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
        if line.startswith("removeprofile"):
            say("# " + line)
    for c in recs:
        say(f"{c['kind']}, {100 * c['fraction']:g} % removed ({c['removed']} rows): remove_ids {c['remove_ms']:.1f} ms; rebuild from host {c['rebuild_ms']:.1f} ms "
            f"({c['rebuild_ms'] / c['remove_ms']:.1f} x); bound {c['bound_ms']:.2f} ms for {c['bytes_moved'] / 1e9:.2f} GB = {100 * c['share_of_bound']:.1f} % of the call; "
            f"first search afterwards {c['first_search_ms']:.1f} ms; distances equal to the rebuilt index: {c['same_distances']}")
    say("json " + json.dumps(recs))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
