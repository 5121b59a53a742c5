#!/usr/bin/env python3
"""reconstruct measurement: reconstruct_batch_device of 1 M random keys at N = 10 M synthetic uniform rows, d = 128, for
Flat, SQ8 and IVF4096,PQ16.

  python3 tools/reconstruct_bench.py [--rows 10000000] [--keys 1000000] [--d 128] [--kinds 'Flat;SQ8;IVF4096,PQ16'] [--out profiles/reconstruct.txt]

Per kind the child reports three figures from the same device in the same run:
  - the call: median ms over 50 timed calls after 3 warm-up calls (HIP events on the caller's stream; the first call, which builds the
    lookup table of a kind with ids, is reported apart), and GB/s of the bytes moved -- the stored rows read plus the f32 rows written;
  - a device-to-device copy of the output's size, timed the same way (GB/s of bytes read plus written);
  - the only route without reconstruct: write_index to a file on tmpfs and reading that file back into memory (once; no parsing, so a lower
    bound of that route).
For the PQ kind it also says which branch of the decode ran (statistic recon_pq_lds).  IVF centroids are 4096 of the rows, codebooks are
random: neither is trained.  The parent process never opens the GPU: the measurement is a child process (--child) under its own time limit."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))


def stored_row_bytes(kind, d):
    if "PQ" in kind:
        return int(kind.split("PQ")[1])
    if "SQ8" in kind:
        return d
    return 4 * d


def child(rows, nkeys, d, kinds):
    import numpy as np
    import torch

    import mi355_faiss as mf

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)

    def timed(fn, warm=3, reps=50):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    keys = torch.from_numpy(rng.integers(0, rows, nkeys).astype(np.int64)).to(dev)
    out = torch.empty((nkeys, d), dtype=torch.float32, device=dev)
    src = torch.rand((nkeys, d), dtype=torch.float32, device=dev)
    cp = timed(lambda: out.copy_(src))
    print("reconjson\t" + json.dumps({"yardstick": "d2d copy", "bytes": 2 * out.numel() * 4, "ms_median": cp[0], "ms_min": cp[1], "ms_max": cp[2],
                                      "GBps": 2 * out.numel() * 4 / cp[0] / 1e6}), flush=True)
    blk = 1 << 20
    for kind in kinds:
        ix = mf.index_factory(d, kind, mf.METRIC_L2)
        if kind.startswith("IVF"):
            nlist = ix.nlist
            ix.ivf_set_centroids(mf.synth_uniform_torch(nlist, d, 7, 0, device=dev).cpu().numpy())
        if "PQ" in kind:
            M = stored_row_bytes(kind, d)
            ix.pq_set_centroids(rng.random((M, 256, d // M), dtype=np.float32))
        if "SQ8" in kind:
            ix.sq_set_trained(np.zeros(d, dtype=np.float32), np.ones(d, dtype=np.float32))
        for r0 in range(0, rows, blk):
            ix.add_torch(mf.synth_uniform_torch(min(blk, rows - r0), d, 7, r0, device=dev))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix.reconstruct_batch_torch(keys, out=out)
        torch.cuda.synchronize()
        first_ms = (time.perf_counter() - t0) * 1e3
        med = timed(lambda: ix.reconstruct_batch_torch(keys, out=out))
        moved = nkeys * (stored_row_bytes(kind, d) + 4 * d)
        rec = {"kind": kind, "rows": rows, "keys": nkeys, "d": d, "first_call_ms": first_ms, "ms_median": med[0], "ms_min": med[1], "ms_max": med[2],
               "bytes_moved": moved, "GBps": moved / med[0] / 1e6, "times_the_copy": med[0] / cp[0]}
        if "PQ" in kind:  # which branch ran, and both branches forced (env MVS_RECON_PQ_LDS, csrc/reconstruct.hip)
            rec["recon_pq_lds"] = ix.get_stat("recon_pq_lds")
            for force in ("0", "1"):
                os.environ["MVS_RECON_PQ_LDS"] = force
                f = timed(lambda: ix.reconstruct_batch_torch(keys, out=out))
                rec["forced_lds_%s" % force] = {"ms_median": f[0], "ms_min": f[1], "ms_max": f[2], "ran": ix.get_stat("recon_pq_lds")}
            del os.environ["MVS_RECON_PQ_LDS"]
        try:
            with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
                p = os.path.join(tmp, "x.index")
                t0 = time.perf_counter()
                mf.write_index(ix, p)
                t1 = time.perf_counter()
                raw = np.fromfile(p, dtype=np.uint8)
                t2 = time.perf_counter()
                rec.update(host_route_write_index_ms=(t1 - t0) * 1e3, host_route_read_file_ms=(t2 - t1) * 1e3, image_bytes=int(raw.size))
                del raw
            rec["host_route_over_call"] = (rec["host_route_write_index_ms"] + rec["host_route_read_file_ms"]) / med[0]
        except (OSError, MemoryError, mf.FaissException) as e:  # (a tmpfs too small for the image: the two device figures stand)
            rec["host_route_error"] = str(e)[:200]
        print("reconjson\t" + json.dumps(rec), flush=True)
        del ix
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--kinds", default="Flat;SQ8;IVF4096,PQ16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    kinds = [k for k in a.kinds.split(";") if k]
    if a.child:
        child(a.rows, a.keys, a.d, kinds)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(a.rows), "--keys", str(a.keys), "--d", str(a.d), "--kinds", a.kinds]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    lines = [l for l in res.stdout.splitlines() if l.startswith("reconjson\t")]
    text = "# tools/reconstruct_bench.py --rows %d --keys %d --d %d --kinds '%s'\n" % (a.rows, a.keys, a.d, a.kinds)
    text += "\n".join(l.split("\t", 1)[1] for l in lines) + "\n"
    sys.stdout.write(text)
    if res.returncode != 0:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        return res.returncode
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
