#!/usr/bin/env python3
"""Selector-program measurement: Flat and IDMap,Flat at N = 10 M synthetic uniform rows, d = 128, L2, searched under
And(Range(half the ids), Not(Batch(1000 ids))).

  python3 tools/selector_bench.py [--rows 10000000] [--d 128] [--kinds 'IDMap,Flat;Flat'] [--nq 64] [--k 10] [--out profiles/selector_bench.txt]

Per kind the child reports
  - the lowering alone: MVS_SELECTOR_PROFILE=1 makes csrc/selector_lower.hip print the time from the program's upload to the plain selector
    being in place, the stream synchronised before and after (the median of the repetitions);
  - the whole filtered search given the program, synchronised (host clock, median);
  - the same search given the equivalent bitmap built on the host, and the time numpy takes to build that bitmap (np.bitwise_or.at over the
    admitted ids, the admitted ids themselves computed by a mask over the id array);
  - whether the two searches agree bit for bit.
What the lowering must move: 8 B per id read (none for a bare Flat index, whose ids are the row numbers) plus ids / 8 bytes of bitmap written;
the scan behind it reads 512 B per row.  The parent process never opens the GPU: the measurement is a child process (--child) under its own
time limit."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))


def child(rows, d, kinds, nq, k, reps):
    import numpy as np
    import torch

    import mi355_faiss as mf

    rng = np.random.default_rng(11)
    xq = mf.synth_uniform_torch(nq, d, 99, 0).cpu().numpy()
    blk = 1 << 20
    for kind in kinds:
        mapped = kind.startswith("IDMap")
        ids = (np.arange(rows, dtype=np.int64) * 2 + 7) if mapped else np.arange(rows, dtype=np.int64)
        ix = mf.index_factory(d, kind, mf.METRIC_L2)
        for r0 in range(0, rows, blk):
            x = mf.synth_uniform_torch(min(blk, rows - r0), d, 7, r0)
            ix.add_torch(x, ids=torch.from_numpy(ids[r0 : r0 + blk]).cuda() if mapped else None)
        lo, hi = int(ids[rows // 4]), int(ids[3 * rows // 4])
        excluded = rng.choice(ids, size=1000, replace=False)
        tree = ("and", ("range", lo, hi), ("not", ("batch", excluded)))
        ix.search(xq, k)  # (derived stores exist, as on an index in use)
        ix.search(xq, k, sel=tree)
        torch.cuda.synchronize()
        t_prog = []
        for _ in range(reps):
            t0 = time.perf_counter()
            Dp, Ip = ix.search(xq, k, sel=tree)
            torch.cuda.synchronize()
            t_prog.append((time.perf_counter() - t0) * 1e3)
        lowered, admitted = ix.get_stat("sel_lowered"), ix.get_stat("sel_admitted")
        t0 = time.perf_counter()
        adm = ids[(ids >= lo) & (ids < hi) & ~np.isin(ids, excluded)]
        bits = np.zeros((int(adm.max()) >> 3) + 1, dtype=np.uint8)
        np.bitwise_or.at(bits, adm >> 3, (1 << (adm & 7)).astype(np.uint8))
        t_host = (time.perf_counter() - t0) * 1e3
        ix.search(xq, k, sel=("bitmap", bits))
        torch.cuda.synchronize()
        t_bitmap = []
        for _ in range(reps):
            t0 = time.perf_counter()
            Db, Ib = ix.search(xq, k, sel=("bitmap", bits))
            torch.cuda.synchronize()
            t_bitmap.append((time.perf_counter() - t0) * 1e3)
        same = bool(np.array_equal(Ip, Ib) and np.array_equal(Dp.view(np.uint32), Db.view(np.uint32)))
        print("json " + json.dumps(dict(kind=kind, rows=rows, d=d, nq=nq, k=k, lowered=int(lowered), admitted=int(admitted), program_search_ms=float(np.median(t_prog)),
                                        bitmap_search_ms=float(np.median(t_bitmap)), host_bitmap_ms=t_host, bitmap_bytes=int(bits.size),
                                        kernel=ix.last_kernel_info()["name"], same=same)), flush=True)
        del ix
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--kinds", default="IDMap,Flat;Flat", help="index strings separated by ';'")
    ap.add_argument("--nq", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    kinds = args.kinds.split(";")
    if args.child:
        return child(args.rows, args.d, kinds, args.nq, args.k, args.reps)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/selector_bench.py: d = {args.d}, N = {args.rows} synthetic uniform rows, L2, nq = {args.nq}, k = {args.k}; And(Range(half the ids), Not(Batch(1000)))")
    say("# lowering: program upload -> plain selector in place, stream synchronised before and after (median); searches: the call + device synchronisation (median)")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(args.rows), "--d", str(args.d), "--kinds", args.kinds, "--nq", str(args.nq),
           "--k", str(args.k), "--reps", str(args.reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, env=dict(os.environ, MVS_SELECTOR_PROFILE="1"))
    except subprocess.TimeoutExpired:
        say(f"NOT COMPLETE (time limit of {args.limit} s)")
        return 1
    if r.returncode != 0:
        say(f"NOT TAKEN (exit status {r.returncode}: {(r.stderr or r.stdout)[-600:]})")
        return 1
    recs = [json.loads(line[5:]) for line in r.stdout.splitlines() if line.startswith("json ")]
    # the child's stderr carries one selprofile line per lowering, in order: per kind 1 warm-up + reps
    prof = [float(m.group(1)) for m in re.finditer(r"selprofile\tlowering of \d+ ids to a \w+: ([0-9.]+) ms", r.stderr)]
    per = 1 + args.reps
    for i, c in enumerate(recs):
        mine = sorted(prof[i * per + 1 : (i + 1) * per])
        c["lowering_ms"] = mine[len(mine) // 2] if mine else None
        low = "not reported" if c["lowering_ms"] is None else f"{c['lowering_ms']:.3f} ms"
        say(f"{c['kind']}: lowered to {('none', 'a bitmap', 'a batch')[c['lowered']]}, {c['admitted']} admitted; lowering alone {low}; search with the program "
            f"{c['program_search_ms']:.2f} ms; search with the host-built bitmap {c['bitmap_search_ms']:.2f} ms + {c['host_bitmap_ms']:.0f} ms to build its "
            f"{c['bitmap_bytes'] / 1e6:.2f} MB in numpy; kernel {c['kernel']}; same results: {c['same']}")
    say("json " + json.dumps(recs))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
