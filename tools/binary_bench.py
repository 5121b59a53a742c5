#!/usr/bin/env python3
"""Hamming scan measurement: BFlat over random codes, k = 10.

  python3 tools/binary_bench.py [--rows 10000000] [--shapes 256:10000,1024:10000,256:1,256:64] [--runs 10] [--out FILE] [--no-baseline]

Per shape (d bits, nq): milliseconds per search -- the median of --runs searches after two warm-up searches, each timed with HIP events
around search_torch with codes and queries resident --, pairs per second, candidates per query (stream records of one search), scan
launches, and the fraction of the popcount ceiling

    ceiling = 1024 SIMDs x 64 lanes x clock / (2 ceil(d / 32) instructions x 2 cycles)  pairs per second.

The clock is the chip's maximum (printed); the 2-cycle issue cost is the guide's figure for v_fma_f32 on a wave64, ASSUMED for v_xor_b32 and
v_bcnt_u32_b32 -- it has not been measured for them.  The fraction is a whole-search figure (scan launches, selection and the host's waits
between generations included), not the scan kernel's own.

For orientation, a same-device baseline: rows and queries expanded to +-1 bf16 (ham = (d - <q, r>) / 2), torch.matmul over row chunks,
torch.topk per chunk and a merge.  The expansion of the rows is not timed.  bf16 sums are exact only up to 256, so at d = 1024 the
baseline's ranking is approximate; it is a speed yardstick, not a reference.  If the expanded rows do not fit, N is reduced for the baseline
and the output says so."""
import argparse
import datetime
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))

K, SIMDS, LANES, CLOCK_HZ, ISSUE_CYCLES = 10, 1024, 64, 2.4e9, 2


def ceiling_pairs_per_s(d):
    return SIMDS * LANES * CLOCK_HZ / (2 * ((d + 31) // 32) * ISSUE_CYCLES)


def random_codes(torch, n, cs, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, (n, cs), dtype=torch.uint8, device="cuda", generator=g)


def timed_runs(torch, fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def expand_pm1(torch, codes):
    """[n, cs] uint8 -> [n, 8 cs] bf16 of +-1 (bit set: +1)"""
    shifts = torch.arange(8, device=codes.device, dtype=torch.uint8)
    bits = (codes.unsqueeze(-1) >> shifts) & 1
    return (bits.reshape(codes.shape[0], -1).to(torch.bfloat16) * 2 - 1).contiguous()


def baseline(torch, rows_pm, xq_pm, d, chunk):
    best_v, best_i = None, None
    for r0 in range(0, rows_pm.shape[0], chunk):
        dots = torch.matmul(xq_pm, rows_pm[r0 : r0 + chunk].T)
        v, i = torch.topk(dots, min(K, dots.shape[1]), dim=1)
        i = i + r0
        if best_v is None:
            best_v, best_i = v, i
        else:
            v2 = torch.cat([best_v, v], dim=1)
            i2 = torch.cat([best_i, i], dim=1)
            best_v, sel = torch.topk(v2, min(K, v2.shape[1]), dim=1)
            best_i = torch.gather(i2, 1, sel)
    return (d - best_v.float()) / 2, best_i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--shapes", default="256:10000,1024:10000,256:1,256:64")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--baseline-runs", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]

    import torch

    import mi355_faiss as mf

    assert mf.device_count() >= 1 and torch.cuda.is_available(), "this tool measures on the GPU: there is none"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/binary_bench.py %s" % " ".join(sys.argv[1:]))
    say("# %s, %s, N = %d random codes, k = %d, median of %d searches after 2 warm-up searches (HIP events)"
        % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0), args.rows, K, args.runs))  # fmt: skip
    say("# ceiling = %d SIMDs x %d lanes x %.2f GHz / (2 ceil(d / 32) x %d cycles); the %d-cycle issue cost is the guide's v_fma_f32 row,"
        % (SIMDS, LANES, CLOCK_HZ / 1e9, ISSUE_CYCLES, ISSUE_CYCLES))  # fmt: skip
    say("# assumed for v_xor_b32 / v_bcnt_u32_b32 (not measured for them); %.2f GHz is the chip's maximum clock, not the clock held under load" % (CLOCK_HZ / 1e9))
    say("%6s %6s %10s %12s %10s %9s %9s %10s | %12s %8s" % ("d", "nq", "ms", "pairs/s", "cand/q", "launches", "rescans", "of ceiling", "baseline ms", "base N"))
    indexes = {}
    for d, nq in shapes:
        cs = d // 8
        if d not in indexes:
            ix = mf.index_binary_factory(d, "BFlat")
            rows = random_codes(torch, args.rows, cs, 1000 + d)
            for r0 in range(0, args.rows, 1 << 20):
                ix.add_torch(rows[r0 : r0 + (1 << 20)].contiguous())
            torch.cuda.synchronize()
            indexes[d] = (ix, rows)
        ix, rows = indexes[d]
        xq = random_codes(torch, nq, cs, 7 + d + nq)
        med, lo, hi = timed_runs(torch, lambda: ix.search_torch(xq, K), args.runs, 2)
        cand, launches, rescans = ix.get_stat("binary_candidates"), ix.get_stat("binary_scan_launches"), ix.get_stat("binary_rescans")
        pairs = nq * args.rows / (med * 1e-3)
        base_ms, base_n = "-", "-"
        if not args.no_baseline:
            try:
                free, _ = torch.cuda.mem_get_info()
                chunk = max(4096, min(1 << 20, (2 << 30) // max(1, nq * 2)))
                bn = args.rows
                while bn * d * 2 * 1.5 + nq * chunk * 8 > free * 0.8 and bn > 1:
                    bn //= 2
                rows_pm = expand_pm1(torch, rows[:bn])  # (not timed)
                xq_pm = expand_pm1(torch, xq)
                bmed, _, _ = timed_runs(torch, lambda: baseline(torch, rows_pm, xq_pm, d, chunk), args.baseline_runs, 1)
                base_ms, base_n = "%.2f" % bmed, ("%d" % bn) + ("" if bn == args.rows else " (reduced: memory)")
                del rows_pm, xq_pm
                torch.cuda.empty_cache()
            except Exception as e:  # the yardstick must not take the measurement down with it
                base_ms, base_n = "failed", type(e).__name__ + ": " + str(e)[:80]
        say("%6d %6d %10.3f %12.4g %10.1f %9d %9d %9.1f%% | %12s %8s   (min %.3f, max %.3f ms)"
            % (d, nq, med, pairs, cand / nq, launches, rescans, 100.0 * pairs / ceiling_pairs_per_s(d), base_ms, base_n, lo, hi))  # fmt: skip
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
