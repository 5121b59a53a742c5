#!/usr/bin/env python3
"""Half-precision Flat measurement: a Flat index and its use_float16 clone, the same queries through both.

  python3 tools/flat16_bench.py [--rows 10000000] [--d 128] [--nq 10000] [--k 10] [--runs 5] [--out profiles/flat16_bench.txt] [--mfma-error]

Per metric (L2, inner product): milliseconds per search of each index -- the median of --runs searches after two warm-up searches, each timed
with HIP events around search_torch with rows and queries resident, the two indexes alternating --; the Flat16 scan kernels' own time (HIP
events around every scan launch of one search, mvs_index_kernel_time_stats) and their share of the dense f16 matrix peak, 2 nq N dpad flops
over that time over 2500 TFLOP/s (the spec figure; the clock held under load is lower); flat16_device_bytes against the Flat index's f32
rows and norms and against everything the Flat index allocated (rows, norms and the filter stores its searches derived); recall@10 of the
Flat16 labels against the Flat labels.  The step time is a whole-search figure: generations, selection and the host's waits included.

--mfma-error: the worst accumulation error of ONE v_mfma_f32_16x16x32_f16 on the tile families of tests/test_mfma_model_gpu.py, in units of
2^-24 x (|C| + sum |a_k b_k|) (what CL_MFMA_UNITS counts for the bf16 instruction) and in ulps of the largest term."""
import argparse
import datetime
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))

PEAK_F16_MFMA_TFLOPS = 2500.0  # v_mfma_f32_16x16x32_f16, dense: the same as the bf16 instruction's


def mfma_error(mf, say):
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_mfma_model_gpu import tiles

    kinds = ["plain", "wide_exponents", "cancellation", "big_c", "small_c", "one_big_term", "same_sign", "big_product_small_terms",
             "big_c_small_terms", "log_uniform"]  # fmt: skip
    say("# v_mfma_f32_16x16x32_f16, one instruction, 4096 tiles per family: worst |D - exact|")
    say("%-26s %14s %18s" % ("family", "u (|C|+sum|ab|)", "ulp(largest term)"))
    worst_all = 0.0
    for kind in kinds:
        rs = np.random.RandomState(sum(map(ord, kind)))
        A, B, C = tiles(kind, 4096, rs)
        Ah, Bh = A.astype(np.float16), B.astype(np.float16)
        D = mf.mfma_f16_16x16x32(Ah.view(np.uint16), Bh.view(np.uint16), C)
        prod = np.einsum("tik,tjk->tijk", Ah.astype(np.float64), Bh.astype(np.float64))  # exact: 22-bit products
        c64 = C.astype(np.float64)
        err = np.abs(D.astype(np.float64) - (prod.sum(-1) + c64))
        mag = np.abs(prod).sum(-1) + np.abs(c64)
        big = np.maximum(np.abs(prod).max(-1), np.abs(c64))
        ulp = np.exp2(np.floor(np.log2(np.maximum(big, 1e-300))) - 23)
        a, b = float((err / (2.0**-24 * np.maximum(mag, 1e-300))).max()), float((err / ulp).max())
        worst_all = max(worst_all, a)
        say("%-26s %14.3f %18.3f" % (kind, a, b))
    say("# worst over the families: %.3f u of (|C| + sum |a b|) per instruction" % worst_all)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--mfma-error", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mi355_faiss as mf

    assert mf.device_count() >= 1 and torch.cuda.is_available(), "this tool measures on the GPU: there is none"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush_out():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    N, d, nq, k = args.rows, args.d, args.nq, args.k
    dpad = (d + 31) // 32 * 32
    say("# tools/flat16_bench.py %s" % " ".join(sys.argv[1:]))
    say("# %s, %s, N = %d uniform rows, d = %d, nq = %d, k = %d; median of %d searches after 2 warm-up searches (HIP events), the two indexes alternating"
        % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0), N, d, nq, k, args.runs))  # fmt: skip
    if args.mfma_error:
        mfma_error(mf, say)
        flush_out()
    say("%-3s %12s %12s %14s %12s %10s | %14s %16s %16s" % ("", "Flat ms", "Flat16 ms", "scan kernels ms", "of f16 peak", "recall@10", "flat16 bytes", "Flat rows+norms", "Flat allocated"))
    xq = mf.synth_uniform_torch(nq, d, 99, 0)
    for name, metric in (("L2", mf.METRIC_L2), ("IP", mf.METRIC_INNER_PRODUCT)):
        flat = mf.index_factory(d, "Flat", metric)
        live0 = flat.get_stat("device_bytes_live")
        for r0 in range(0, N, 1 << 20):
            nb = min(1 << 20, N - r0)
            flat.add_torch(mf.synth_uniform_torch(nb, d, 1, r0))
        torch.cuda.synchronize()
        half = flat.clone_to_gpu(0, use_float16=True)
        f16_bytes = half.get_stat("flat16_device_bytes")
        ms = {"flat": [], "half": []}
        out = {}
        for run in range(args.runs + 2):
            for key, ix in (("flat", flat), ("half", half)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out[key] = ix.search_torch(xq, k)
                b.record()
                torch.cuda.synchronize()
                if run >= 2:
                    ms[key].append(a.elapsed_time(b))
        flat_alloc = flat.get_stat("device_bytes_live") - live0 - f16_bytes
        half.set_kernel_timing(True)
        c0, t0 = half.kernel_time_stats()
        half.search_torch(xq, k)
        torch.cuda.synchronize()
        c1, t1 = half.kernel_time_stats()
        half.set_kernel_timing(False)
        scan_ms = t1 - t0
        frac = 2.0 * nq * N * dpad / (scan_ms * 1e-3) / 1e12 / PEAK_F16_MFMA_TFLOPS
        If, Ih = out["flat"][1].cpu().numpy(), out["half"][1].cpu().numpy()
        recall = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(If, Ih)) / float(If.size)
        say("%-3s %12.2f %12.2f %14.2f %11.1f%% %10.4f | %14d %16d %16d   (Flat min %.2f max %.2f, Flat16 min %.2f max %.2f ms; %d scan launches, %.1f candidates per query; Flat kernel %s)"
            % (name, statistics.median(ms["flat"]), statistics.median(ms["half"]), scan_ms, 100.0 * frac, recall, f16_bytes, N * (4 * d + 4),
               flat_alloc, min(ms["flat"]), max(ms["flat"]), min(ms["half"]), max(ms["half"]), c1 - c0, half.get_stat("flat16_candidates") / nq,
               flat.last_kernel_info()["name"]))  # fmt: skip
        flush_out()
        del flat, half, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
