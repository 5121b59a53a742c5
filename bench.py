#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X vector-search hot path.

Metric (BASELINE.json): queries/sec (+ recall@10), FlatL2 d=128 N=10M nq=10k k=10, at 1/2/4/8 MI355X.

One "step" = one pass of the hot path over one batch: all nq queries searched against the whole database
(Index::search, /root/reference/src/faiss_extension.cpp:631), inputs already resident in HBM.
With --gpus N the database is ROW-SHARDED over the N ranks (fixed total N => strong scaling); each step is
local search -> RCCL all-gather of the per-shard (distance,label) blocks -> host k-way merge on rank 0
(SURVEY.md 8e).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the steps and prints the line; --full adds every other measurement and check (CPU
baselines and oracle checks, recall, HBM copy rate, state sensitivity; on the headline workload the host-pointer timing,
ingest cases and embedded configs) and takes a few minutes.  --dump-outputs DIR writes the last timed step's results.

    python bench.py                      # N=1, the headline figure only
    python bench.py --full               # ... and everything else
    python bench.py --dump-outputs out   # out/distances.npy, out/labels.npy: to compare two builds result for result
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        --master-port 29500 bench.py --gpus 8 --steps 5 --warmup 1
"""
import argparse
import json
import os
import sys
import time

# the CPU-baseline leg alternates OpenBLAS's pthreads with the oracle's OpenMP loops: spinning OpenMP workers would starve the sgemm
os.environ.setdefault("OMP_WAIT_POLICY", "passive")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "duckdb-faiss-ext_amd", "pyhost"))

PEAK_F32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_bf16, dense (spec; ~2.0 PF at the clock it holds)
PEAK_HBM_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E spec (6.29 TB/s measured copy)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", "--rows", dest="n", type=int, default=10_000_000)  # --rows: torchrun's parser trips over "--n"
    ap.add_argument("--d", "--dim", dest="d", type=int, default=128)  # --dim: torchrun's parser takes "--d" for one of its own
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", default="L2", choices=["L2", "IP"])
    ap.add_argument("--index", default="Flat", help="factory string (Flat | IDMap,Flat | IVF4096,Flat ...)")
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--efsearch", type=int, default=128, help="SearchParametersHNSW::efSearch (HNSW indexes)")
    ap.add_argument("--no-pipeline", action="store_true", help="N > 1: merge every batch before searching the next")
    ap.add_argument("--efconstruction", type=int, default=0, help="hnsw.efConstruction (0 = FAISS default 40)")
    ap.add_argument("--normalize", action="store_true", help="L2-normalise rows and queries (embedding-like, C4/C5)")
    ap.add_argument("--chunk", type=int, default=0, help="queries per search call (2048 = DuckDB DataChunk); 0 = one batch")
    ap.add_argument("--cpu-seconds", type=float, default=30.0, help="--full: CPU-baseline budget (rank 0, N=1 only)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines and oracle checks")
    ap.add_argument("--opt", action="append", default=[], help="index option key=value (e.g. ivf_mfma=1)")
    ap.add_argument("--data", default="uniform", choices=["uniform", "clustered"])
    ap.add_argument("--centers", type=int, default=1024, help="clustered data: number of mixture centres")
    ap.add_argument("--sigma", type=float, default=0.1, help="clustered data: per-coordinate spread around a centre")
    ap.add_argument("--query-groups", type=int, default=1, help="N > 1, Flat / IVF: G groups of N / G row shards, group g answers the "
                    "g-th slice of the queries (default 1 = the north-star layout: 1 x N row shards, the database stored once)")
    ap.add_argument("--secondary", action="store_true", help="N > 1 headline run: after the timed region rank 0 also runs the secondary "
                    "layouts (2 query groups x N/2 row shards; the in-library ShardedIndex in one process) as child launches and adds them "
                    "to its line.  Opt-in (ADVICE r4): a driver time limit hit while the children run must not cost the headline its line")
    ap.add_argument("--no-secondary", action="store_true", help=argparse.SUPPRESS)  # (round 4's flag: the default now)
    ap.add_argument("--no-ingest", action="store_true", help="--full headline run: skip the ingest lines (host/boundary_driver ingest)")
    ap.add_argument("--inlib-shards", type=int, default=0, help="one process, --gpus 1: spread the index over this many devices INSIDE "
                    "the library (csrc/sharded.hip, what faiss_to_gpu(name, -1) / MVS_DEVICES do) and time Index::search on it")
    ap.add_argument("--no-configs", action="store_true", help="--full headline run: skip the embedded C2/C3/C4-shard/C5 lines")
    ap.add_argument("--no-host-pointer", action="store_true", help="--full headline run: skip the pageable-host-pointer timing")
    ap.add_argument("--parity-device", type=int, default=0, help="re-run this many queries on the exact device kernel "
                    "(Flat: f32 MFMA kernel, IVF: scanner kernel -- both oracle-checked in tests/) and compare bit for bit")
    ap.add_argument("--full", action="store_true", help="after the timed steps also measure and check everything beyond the headline "
                    "figure: CPU baselines and oracle checks, recall, the HBM copy rate, the state-sensitivity searches and, on the "
                    "headline workload, the host-pointer timing, the ingest cases and the embedded configs (off: set up, warm up, time "
                    "the steps, print the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the results of the last timed step (what a caller of "
                    "the search receives) to DIR/distances.npy (float32) and DIR/labels.npy (float64), at most 64 MB in all: beyond "
                    "that a fixed, seeded sample of query rows, whose indices go to DIR/query_rows.npy")
    return ap.parse_args()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, D, I):
    """--dump-outputs: the (distances, labels) of the last timed step as .npy, float32 / float64 (labels are integers below 2^53, so
    float64 holds them exactly).  Larger than DUMP_LIMIT_BYTES: a fixed sample of query rows (seed 0, sorted), the same for the same
    arguments, so two builds compare row for row."""
    import numpy as np

    D = np.asarray(D, dtype=np.float32)
    I = np.asarray(I).astype(np.float64)
    rows = None
    if D.nbytes + I.nbytes > DUMP_LIMIT_BYTES:
        per_row = D.shape[1] * 4 + I.shape[1] * 8 + 8  # (+ its entry in query_rows.npy)
        keep = max(1, (DUMP_LIMIT_BYTES - 4096) // per_row)  # (4 KB for the three .npy headers)
        rows = np.sort(np.random.default_rng(0).choice(D.shape[0], size=min(keep, D.shape[0]), replace=False))
        D, I = D[rows], I[rows]
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "distances.npy"), np.ascontiguousarray(D))
    np.save(os.path.join(dirname, "labels.npy"), np.ascontiguousarray(I))
    if rows is not None:
        np.save(os.path.join(dirname, "query_rows.npy"), rows.astype(np.float64))


def host_pointer_timing(ix, xq, k, np, time):
    """The call the glue makes (src/faiss_extension.cpp:626-631): Index::search(n, x, k, D, I) with PAGEABLE host pointers --
    queries H2D and results D2H are inside the time.  One 10k batch and DuckDB's 2048-row chunks (:903-925)."""
    xq_h = np.ascontiguousarray(xq.cpu().numpy())
    nq = xq_h.shape[0]
    res = {"api": "mvs_index_search, pageable numpy buffers (queries H2D + results D2H inside the time)"}
    for name, chunk in (("single_batch", nq), ("chunks_2048", 2048)):
        best = None
        for rep in range(4):  # first = warm-up (staging buffers), best of the next 3
            t0 = time.perf_counter()
            for q0 in range(0, nq, chunk):
                ix.search(xq_h[q0 : q0 + chunk], k)
            dt = time.perf_counter() - t0
            if rep > 0:
                best = dt if best is None else min(best, dt)
        res[name] = {"queries_per_call": chunk, "ms_per_batch": round(best * 1e3, 3), "value": round(nq / best, 1), "unit": "queries/s"}
    return res


_LAUNCH_ENV = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "GROUP_WORLD_SIZE", "ROLE_RANK", "ROLE_NAME",
               "ROLE_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "OMP_NUM_THREADS", "MVS_DEVICE")


def _child_env():
    """environment for a child launch: nothing of an enclosing torchrun (a nested launch must make its own rendezvous)"""
    env = {k: v for k, v in os.environ.items() if k not in _LAUNCH_ENV and not k.startswith("TORCHELASTIC_") and not k.startswith("TORCH_NCCL_")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this pool: RCCL needs it
    return env


def _free_port():
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(gpus, argv, timeout=None):
    """`python bench.py --gpus N` with no launcher around it: start the N ranks -- one process per GPU -- as CHILD processes
    (torch.distributed.run on 127.0.0.1, a free port) and hand back rank 0's JSON line.  The caller has not touched the GPU
    (or, for the secondary layouts, is a finished rank 0 whose children are ordinary child processes, never an exec).
    -> (return code, JSON line or None, tail of the children's stderr)"""
    import subprocess

    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    import signal

    # (its own process group: a launch that outlives its time limit is ended as a whole -- launcher and ranks -- by the group id we
    # created, so that no rank stays behind holding a GPU)
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=_child_env(), start_new_session=True)
    try:
        so, se = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except OSError:
            pass
        so, se = p.communicate()
        return 124, None, "timed out after %s s: %s" % (timeout, (se or "")[-300:])
    lines = [l for l in so.splitlines() if l.startswith("{")]
    return p.returncode, (lines[-1] if lines else None), (se or "")[-2000:]


def secondary_layouts(args, world):
    """The same headline step on the other two ways this tree spreads a Flat index over the node's GPUs, as child launches of a
    FINISHED rank 0 (every rank has freed its GPU): (i) 2 query groups x N/2 row shards (the database stored twice), (ii) ONE
    process, the in-library ShardedIndex (csrc/sharded.hip -- what a DuckDB process gets from faiss_to_gpu(name, -1) / MVS_DEVICES).
    `value` of the line stays the north-star layout: 1 x N row shards."""
    import subprocess

    common = ["--steps", str(args.steps), "--warmup", str(args.warmup), "--rows", str(args.n), "--dim", str(args.d), "--nq", str(args.nq),
              "--k", str(args.k), "--metric", args.metric, "--no-secondary", "--no-cpu-baseline", "--no-configs", "--no-host-pointer"]
    res = {}

    def digest(j):
        return {"value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "n_gpus": j["n_gpus"],
                "row_shards": j["config"].get("row_shards"), "replicas": j["config"].get("replicas"),
                "merged_labels_bit_exact_vs_oracle": j.get("merged_labels_bit_exact_vs_oracle"), "exchange": j["config"].get("exchange")}

    if world >= 4 and world % 2 == 0 and args.metric == "L2":
        t0 = time.perf_counter()
        try:
            rc, line, err = launch_ranks(world, ["--gpus", str(world), "--query-groups", "2"] + common, timeout=200)
            res["query_groups_2"] = digest(json.loads(line)) if rc == 0 and line else {"error": "rc=%d %s" % (rc, err[-300:])}
        except Exception as ex:  # noqa: BLE001  (a secondary entry must never cost the run its line)
            res["query_groups_2"] = {"error": repr(ex)[:300]}
        res["query_groups_2"]["seconds"] = round(time.perf_counter() - t0, 1)
    t0 = time.perf_counter()
    try:
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--inlib-shards", str(world)] + common
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=200, env=_child_env())
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        res["in_library_sharded_index"] = digest(json.loads(line[-1])) if p.returncode == 0 and line else {"error": (p.stderr or p.stdout)[-300:]}
    except Exception as ex:  # noqa: BLE001
        res["in_library_sharded_index"] = {"error": repr(ex)[:300]}
    res["in_library_sharded_index"]["seconds"] = round(time.perf_counter() - t0, 1)
    return res


EMBEDDED = [  # (name, workload of BASELINE.json configs[i], bench.py arguments)
    ("C2", "IndexFlatL2 d=128 N=1M nq=10k k=10", ["--rows", "1000000", "--cpu-seconds", "4", "--steps", "10", "--warmup", "2"]),
    # (round 6, VERDICT r5 #4 / #5: one GPU's row shard of the headline on 8 GPUs -- the number the >= 6 x claim hangs on -- and the
    # headline under the reference's DEFAULT metric, src/faiss_extension.cpp:105)
    ("H_shard8", "IndexFlatL2 d=128, one GPU's N/8 = 1.25M rows of N=10M, nq=10k k=10",
     ["--rows", "1250000", "--cpu-seconds", "4", "--parity-device", "1024", "--steps", "10", "--warmup", "2"]),
    ("H_IP", "IndexFlatIP d=128 N=10M nq=10k k=10 (faiss_create's default metric)",
     ["--metric", "IP", "--no-cpu-baseline", "--parity-device", "1024", "--steps", "5", "--warmup", "1"]),
    # (round 6, VERDICT r5 missing #3: the list lengths of the reference's post-filter use, README.md:222-271 / go/main_test.go:26-32)
    ("H_k1000", "IndexFlatL2 d=128 N=10M nq=2048 k=1000 (post-filter list length)",
     ["--nq", "2048", "--k", "1000", "--no-cpu-baseline", "--parity-device", "64", "--steps", "3", "--warmup", "1"]),
    ("C3", "IVF4096,Flat d=128 N=10M nprobe=32 nq=10k k=10", ["--index", "IVF4096,Flat", "--data", "clustered", "--parity-device", "1024", "--steps", "10", "--warmup", "2"]),
    ("C3_k100", "IVF4096,Flat d=128 N=10M nprobe=32 nq=2048 k=100 (list length beyond the scan's class slots)",
     ["--index", "IVF4096,Flat", "--data", "clustered", "--nq", "2048", "--k", "100", "--no-cpu-baseline", "--parity-device", "64", "--steps", "5", "--warmup", "2"]),
    ("C4_shard", "IndexFlatIP d=768, one GPU's N/8 = 12.5M rows of N=100M, nq=10k k=10",
     ["--rows", "12500000", "--d", "768", "--metric", "IP", "--normalize", "--data", "clustered", "--sigma", "1.0", "--cpu-seconds", "8", "--parity-device", "256"]),
    ("C5", "IDMap,HNSW32 d=768 N=1M nq=10k k=10 efSearch=128",
     ["--index", "IDMap,HNSW32", "--rows", "1000000", "--d", "768", "--normalize", "--data", "clustered", "--sigma", "1.0", "--cpu-seconds", "2"]),
]


INGEST = [  # (name, boundary_driver ingest arguments: rows, d, threads, index) -- VERDICT r4 #8
    ("flat_10m_d128", ["10000000", "128", "8", "IDMap,Flat"]),
    ("ivf4096_10m_d128", ["10000000", "128", "8", "IVF4096,Flat"]),
    ("hnsw32_500k_d768", ["500000", "768", "8", "IDMap,HNSW32"]),
]


def ingest_lines():
    """the glue's ingest call pattern (src/faiss_extension.cpp:475-547 AddFunction: <= 2048-row DataChunks from
    several threads under faiss_lock; :549-615 AddFinalise: train on all rows, add the rest) through the faiss:: adaptor, by
    host/boundary_driver as a child process: rows/s, GB/s of row data and the fraction of this box's measured host-to-device
    copy rate (pinned).  IVF includes its k-means training, HNSW its graph build."""
    import subprocess

    exe = os.path.join(ROOT, "duckdb-faiss-ext_amd", "host", "boundary_driver")
    if not os.path.exists(exe):
        return {"error": "host/boundary_driver is not built"}
    res = {}

    def run(argv, tag, timeout):
        p = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=timeout)
        for l in p.stdout.splitlines():
            if l.startswith(tag + "\t"):
                return json.loads(l.split("\t", 1)[1]), p
        return None, p

    try:
        link, p = run(["linkrate"], "linkjson", 120)
        res["link"] = link if link else {"error": (p.stderr or p.stdout)[-200:]}
    except Exception as e:  # noqa: BLE001
        res["link"] = {"error": repr(e)[:200]}
    pinned = (res["link"] or {}).get("h2d_pinned_GBps")
    for name, argv in INGEST:
        t0 = time.perf_counter()
        try:
            j, p = run(["ingest"] + argv, "ingestjson", 300)
            if j is None or p.returncode != 0:
                res[name] = {"error": (p.stderr or p.stdout)[-300:], "rc": p.returncode}
                continue
            j["frac_of_h2d_pinned"] = round(j["GBps"] / pinned, 4) if pinned else None
            if "HNSW" in j["index"]:
                j["note"] = ("the driver's rows are UNIFORM random: the hardest case for a graph build (no structure, long walks) -- C5's clustered "
                             "normalised rows build an order of magnitude faster: configs.C5.build_seconds for its 1 M rows")
            if "IVF" in j["index"]:
                j["note"] = "includes AddFinalise's k-means training on all rows (src/faiss_extension.cpp:583) and the list build"
            j["call_pattern"] = "add calls of <= 2048 rows (pageable buffers valid only during the call) from %d threads" % j["threads"]
            j["child_seconds"] = round(time.perf_counter() - t0, 1)
            res[name] = j
        except Exception as e:  # noqa: BLE001
            res[name] = {"error": repr(e)[:200]}
    return res


def embedded_configs():
    """C2 / C3 / C4-shard / C5 for 3 steps each, as child processes of the headline run: the driver-timed line
    then carries every BASELINE config.  A child that fails or times out reports its error instead of a number."""
    import subprocess

    res = {}
    for name, workload, extra in EMBEDDED:
        t0 = time.perf_counter()
        # (3 steps unless the config says otherwise: the short ones take 10 -- their first searches size buffers and estimates)
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-configs",
               "--no-host-pointer"] + extra
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")]
            if p.returncode != 0 or not line:
                res[name] = {"workload": workload, "error": (p.stderr or p.stdout)[-300:]}
                continue
            j = json.loads(line[-1])
            r = j.get("roofline", {})
            e = {
                "workload": workload,
                "value": j["value"],
                "unit": j["unit"],
                "ms_per_step": j["ms_per_step"],
                "steps": j["steps"],
                "build_seconds": j.get("config", {}).get("build_seconds"),
                "roofline": {kk: r.get(kk) for kk in ("kernel", "bound", "achieved", "peak", "unit", "frac", "frac_step", "avg_launch_ms",
                                                      "frac_counter", "mfma_busy_frac", "list_major_bytes_8d", "candidates_rescored_per_query",
                                                      "candidates_admitted_per_query", "probe_pairs", "probe_pairs_scanned", "scan_forced_drains", "traffic",
                                                      "traffic_over_algorithmic", "row_bytes_moved_GBps")},
                "parity": {kk: j[kk] for kk in ("labels_bit_exact_vs_oracle", "labels_and_distances_bit_exact_vs_oracle", "parity_device",
                                                "recall_at_10", "recall_sample_queries", "labels_equal_vs_openblas", "openblas_census",
                                                "hnsw_pop_min_tie_rule") if kk in j},
                "seconds": round(time.perf_counter() - t0, 1),
            }
            for kk in ("cpu_baseline", "cpu_baseline_port", "cpu_baseline_openblas", "recall_efConstruction_200"):
                if kk in j:
                    e[kk] = j[kk]
            res[name] = e
        except Exception as ex:  # noqa: BLE001  (never let an extra line cost the headline its bench line)
            res[name] = {"workload": workload, "error": repr(ex)[:300]}
    return res


def _cfg_digest(e):
    """<= 300 bytes per embedded config: what the driver's record must show for it."""
    if "error" in e:
        return {"error": str(e["error"])[-120:]}
    r, par = e.get("roofline") or {}, e.get("parity") or {}
    pd = par.get("parity_device") or {}
    g = {"qps": e.get("value"), "ms": e.get("ms_per_step"), "kernel": r.get("kernel"), "bound": r.get("bound"), "frac": r.get("frac"),
         "frac_step": r.get("frac_step")}
    if r.get("traffic_over_algorithmic") is not None:
        g["traffic_x"] = r["traffic_over_algorithmic"]
    for kk, short in (("labels_bit_exact_vs_oracle", "labels=oracle"), ("labels_and_distances_bit_exact_vs_oracle", "bits=oracle"),
                      ("labels_equal_vs_openblas", "labels=openblas"), ("recall_at_10", "recall@10")):
        if kk in par:
            g[short] = par[kk]
    if pd:
        g["bits=exact_kernel"] = bool(pd.get("labels_equal") and pd.get("distances_bit_equal"))
    cb = e.get("cpu_baseline")
    if cb:
        g["cpu_qps"] = cb.get("value")
    return g


def compact_line(out):
    """The ONE line rank 0 prints stays short enough for the driver's record (BENCH_r05.json kept 2 KB of parsed keys and an 8 KB
    stdout tail: C3 and C4 were cut off).  Every embedded config and ingest case goes into `config` as a digest; long strings, sweeps
    and the full per-config entries go to the sidecar gpurun_out/bench_detail.json (and profiles/ when committed)."""
    detail = json.loads(json.dumps(out))
    line = dict(out)
    cfg = dict(line.get("config") or {})
    if "configs" in line:
        cfg["configs"] = {name: _cfg_digest(e) for name, e in line.pop("configs").items()}
    if "ingest" in line:
        ing = line.pop("ingest")
        cfg["ingest"] = {name: ({"rows_per_s": e.get("rows_per_s"), "GBps": e.get("GBps"), "frac_h2d": e.get("frac_of_h2d_pinned")}
                                if isinstance(e, dict) and "error" not in e and name != "link" else e) for name, e in ing.items()}
    if isinstance(cfg.get("collective"), dict) and len(json.dumps(cfg["collective"])) > 200:  # (per-rank device lists -> detail)
        cfg["collective"] = {x: cfg["collective"].get(x) for x in ("backend", "world_size", "allreduce_of_ones", "distinct_devices")}
    for kk in ("state_sensitivity", "options"):
        if kk in cfg and cfg[kk] and len(json.dumps(cfg[kk])) > 200:
            cfg[kk] = "see detail"
    line["config"] = cfg
    r = dict(line.get("roofline") or {})
    for kk in ("traffic_source", "traffic_note", "mfma_busy_source"):
        r.pop(kk, None)
    if r:
        line["roofline"] = r
    cb = dict(line.get("cpu_baseline") or {})
    for kk in ("cores_note", "thread_sweep_qps", "selected"):
        cb.pop(kk, None)
    if "sample" in cb and len(cb["sample"]) > 160:
        cb["sample"] = cb["sample"][:157] + "..."
    if cb:
        line["cpu_baseline"] = cb
    for kk in ("cpu_baseline_port", "cpu_baseline_openblas", "cpu_sgemm_upper_bound", "openblas_census", "host_pointer", "secondary"):
        if kk in line and len(json.dumps(line[kk])) > 150:
            v = line.pop(kk)
            if isinstance(v, dict) and "value" in v:
                line[kk] = {x: v[x] for x in ("value", "unit", "cores", "tflops") if x in v}
            elif kk == "openblas_census":
                line[kk] = {x: v[x] for x in ("slots", "slots_label_differs", "slots_outside_band") if x in v}
            elif kk == "secondary":
                line[kk] = {n_: {x: e.get(x) for x in ("value", "ms_per_step", "error") if x in e} for n_, e in v.items()}
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "bench_detail.json"), "w") as f:
            f.write(json.dumps(detail) + "\n")
        line["detail"] = "gpurun_out/bench_detail.json"
    except OSError:
        line["detail"] = None
    return line


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher around us: start the N ranks ourselves, as child processes, BEFORE anything here touches the GPU, and relay
        # rank 0's line (the explicit `python -m torch.distributed.run ... bench.py --gpus N` form keeps working: it sets WORLD_SIZE)
        rc, line, err = launch_ranks(args.gpus, sys.argv[1:])
        if line:
            print(line, flush=True)
        if rc != 0 or not line:
            sys.stderr.write(err)
        raise SystemExit(rc if rc != 0 else (0 if line else 1))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        args.gpus = world
    # debugging aid for the N > 1 flow on a 1-GPU box: MVS_BENCH_SHARED_GPU=1 MVS_BENCH_BACKEND=gloo puts every rank
    # on device 0 (RCCL refuses two ranks on one GPU); never set by the driver, numbers from it mean nothing
    if os.environ.get("MVS_BENCH_SHARED_GPU") == "1":
        local_rank = 0
    backend = os.environ.get("MVS_BENCH_BACKEND", "nccl")
    os.environ["MVS_DEVICE"] = str(local_rank)

    import numpy as np
    import torch
    import torch.distributed as dist

    import mi355_faiss as mf

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    # what the collective library saw: every rank reports its device; rank 0 prints the census (VERDICT r4 #5c)
    ranks_seen = None
    if world > 1:
        try:
            props = torch.cuda.get_device_properties(local_rank)
            me = {"rank": rank, "local_rank": local_rank, "device": local_rank, "name": props.name,
                  "pci_bus_id": getattr(props, "pci_bus_id", None), "uuid": str(getattr(props, "uuid", "")) or None,
                  "pid": os.getpid()}
            gathered = [None] * world
            dist.all_gather_object(gathered, me)
            probe = torch.ones(1, dtype=torch.int64, device=dev)
            dist.all_reduce(probe)  # one collective on the data-path backend: its result IS the number of ranks it spans
            ranks_seen = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "allreduce_of_ones": int(probe.item()),
                          "distinct_devices": len({(g["pci_bus_id"], g["uuid"], g["device"]) for g in gathered}), "ranks": gathered}
        except Exception as e:  # noqa: BLE001
            ranks_seen = {"error": repr(e)[:200]}

    metric = mf.METRIC_L2 if args.metric == "L2" else mf.METRIC_INNER_PRODUCT
    n, d, nq, k = args.n, args.d, args.nq, args.k
    # N ranks = G query groups x R row shards (rank = g * R + shard); G = 1: row shards only.  A shard's step has a part per (query,
    # row) pair and a part per query (candidates while the bound converges, exact re-scoring, select): at 8 ranks 2 x 4 halves the
    # second.  The inner-product tie protocol (below) and the HNSW replicas keep G = 1.
    qgroups = max(1, args.query_groups)  # `value` is always BASELINE's layout (row shards only); 2 x N/2 is a secondary entry
    if "HNSW" in args.index and "IVF" not in args.index:
        qgroups = 1
    if world % qgroups != 0 or (qgroups > 1 and args.metric != "L2" and "IVF" not in args.index):
        raise SystemExit("--query-groups must divide --gpus (Flat inner product: 1)")
    nshards = world // qgroups
    # row shard of this rank: [r0, r1)
    r0, r1 = n * (rank % nshards) // nshards, n * (rank % nshards + 1) // nshards
    DB_SEED, Q_SEED = 1234, 4321

    if args.data == "uniform":
        gen = mf.synth_uniform_torch
    else:

        def gen(m, dd, seed, row0=0, device=None):
            return mf.synth_clustered_torch(m, dd, seed, row0=row0, n_centers=args.centers, sigma=args.sigma, device=device)

    ix = mf.index_factory(d, args.index, metric)
    for o in args.opt:
        key, v = o.split("=")
        ix.set_option(key, int(v))
    is_ivf = "IVF" in args.index
    is_hnsw = "HNSW" in args.index
    if is_hnsw and not is_ivf and args.efconstruction > 0:
        ix.set_ef_construction(args.efconstruction)
    with_ids = args.index.startswith("IDMap")
    if is_hnsw:
        # the graph walk does not shard -> replicas only: every rank holds the whole graph + vectors and
        # answers its slice of the queries; no data-path collective (rank 0 gathers the disjoint result rows)
        r0, r1 = 0, n

    def prep(x):
        if args.normalize:
            x /= x.norm(dim=1, keepdim=True)
        return x

    if not with_ids:
        ix.set_label_offset(r0)  # global labels of this row shard (IVF stores them at add time)
    def host_rows(count, seed):
        """the same rows on the host for the oracle: the host generator (bit-identical to the device one) or, when the
        rows are normalised on the device, a copy of exactly those"""
        from oracle import oracle as orc

        if not args.normalize:
            if args.data == "uniform":
                return orc.synth_uniform(count, d, seed)
            return orc.synth_clustered(count, d, seed, n_centers=args.centers, sigma=args.sigma)
        out_h = np.empty((count, d), dtype=np.float32)
        for s0 in range(0, count, 1 << 20):
            m = min(1 << 20, count - s0)
            out_h[s0 : s0 + m] = prep(gen(m, d, seed, row0=s0, device=dev)).cpu().numpy()
        return out_h

    # build: device-side generation in slabs (keeps peak memory = index + one slab)
    slab = 1 << 20
    t_build0 = time.time()
    if is_ivf:
        # the reference trains on ALL rows it was given (src/faiss_extension.cpp:583) and then adds them (:609)
        # N > 1: rank 0 trains on its rows, the centroids are replicated, every list is row-sharded
        from sharded import replicate_ivf_centroids

        xb_all = gen(r1 - r0, d, DB_SEED, row0=r0, device=dev)
        if world > 1 and rank == 0:
            # the centroids must be those of the 1-GPU run: rank 0 trains on ALL N rows (FAISS subsamples 256 per
            # centroid out of them with its own RNG), not on its shard
            x_train = np.empty((n, d), dtype=np.float32)
            for s0 in range(0, n, slab):
                m = min(slab, n - s0)
                x_train[s0 : s0 + m] = gen(m, d, DB_SEED, row0=s0, device=dev).cpu().numpy()
        else:
            x_train = xb_all.cpu().numpy() if rank == 0 else None
        replicate_ivf_centroids(ix, x_train, src=0, device=dev)
        del x_train
        for s0 in range(0, r1 - r0, slab):
            ix.add_torch(xb_all[s0 : s0 + slab])
        torch.cuda.synchronize()
    else:
        if is_hnsw:
            slab = 1 << 16
        for s0 in range(r0, r1, slab):
            m = min(slab, r1 - s0)
            xb = prep(gen(m, d, DB_SEED, row0=s0, device=dev))
            ids = torch.arange(s0, s0 + m, dtype=torch.int64, device=dev) if with_ids else None
            ix.add_torch(xb, ids=ids)
            torch.cuda.synchronize()
            del xb
    xq = prep(gen(nq, d, Q_SEED, row0=0, device=dev))
    torch.cuda.synchronize()
    if args.inlib_shards > 1:
        # ONE process, the index spread over the node's GPUs inside the library (row shards; peer copies + device merge)
        if world != 1:
            raise SystemExit("--inlib-shards is a one-process layout (--gpus 1)")
        shared = os.environ.get("MVS_BENCH_SHARED_GPU") == "1"
        if not shared and mf.device_count() < args.inlib_shards:
            raise SystemExit("--inlib-shards %d: only %d devices visible" % (args.inlib_shards, mf.device_count()))
        ix.shard_to_gpus([0 if shared else g for g in range(args.inlib_shards)])
    t_build = time.time() - t_build0

    from sharded import ShardExchange

    # Row shards + inner product: FAISS's CMin heap resolves exact ties at the k-th score by arrival order, so the shards
    # hand over k + 1 candidates in the pure order and rank 0 runs the tie protocol (pyhost/sharded.py); L2 is a pure
    # function of the data and needs neither.
    ip_ties = world > 1 and metric == mf.METRIC_INNER_PRODUCT and not is_ivf and not is_hnsw and not with_ids
    # Row-sharded IVF (round 5): FAISS's scanner heap keeps rows tied at the k-th value by ARRIVAL order (probe rank, list position):
    # the shards hand over k + 1 entries in the pure order and rank 0 runs the cross-process protocol (pyhost/sharded.py
    # merge_ivf_exact) -- the path `bench.py --gpus N --index IVF...` times is the bit-exact one (VERDICT r4 missing #2)
    ivf_ties = world > 1 and is_ivf and not with_ids and qgroups == 1 and args.chunk in (0, nq)  # (the tie pass reuses the batch's coarse assignment)
    ks = k + 1 if (ip_ties or ivf_ties) else k
    if ip_ties:
        ix.set_option("ip_exact_ties", 0)
    if ivf_ties:
        ix.set_option("ivf_exact_ties", 0)
    D = torch.empty((nq, ks), dtype=torch.float32, device=dev)
    I = torch.empty((nq, ks), dtype=torch.int64, device=dev)
    # N > 1: two result / exchange buffer sets, so that the host merge of batch i runs while the GPUs search batch i+1
    pipelined = world > 1 and not is_hnsw and not args.no_pipeline and not ip_ties and not ivf_ties
    Dbuf, Ibuf = [D], [I]
    xchs = [ShardExchange(nq, k, dev, ip_ties=ip_ties or ivf_ties, metric=metric, qgroups=qgroups)]
    if pipelined:
        Dbuf.append(torch.empty_like(D))
        Ibuf.append(torch.empty_like(I))
        xchs.append(ShardExchange(nq, k, dev, metric=metric, qgroups=qgroups))
    gq0, gq1 = xchs[0].query_range()  # the queries this rank answers (all of them with one query group)
    state = {"it": 0, "pending": None}
    chunk = args.chunk if args.chunk > 0 else nq
    search_kw = {"nprobe": args.nprobe} if is_ivf else ({"efSearch": args.efsearch} if is_hnsw else {})
    final = {}
    # replicas: rank r answers queries [qa, qb)
    per = (nq + world - 1) // world
    qa, qb = min(nq, rank * per), min(nq, (rank + 1) * per)

    def step_replicas():
        if qb > qa:
            ix.search_torch(xq[qa:qb], k, D=D[qa:qb], I=I[qa:qb], **search_kw)
        if world > 1:
            Dl = torch.zeros((per, k), dtype=torch.float32, device=dev)
            Il = torch.full((per, k), -1, dtype=torch.int64, device=dev)
            Dl[: qb - qa], Il[: qb - qa] = D[qa:qb], I[qa:qb]
            Dg = torch.empty((world * per, k), dtype=torch.float32, device=dev)
            Ig = torch.empty((world * per, k), dtype=torch.int64, device=dev)
            dist.all_gather_into_tensor(Dg, Dl)
            dist.all_gather_into_tensor(Ig, Il)
            if rank == 0:
                final["D"], final["I"] = Dg[:nq].cpu().numpy(), Ig[:nq].cpu().numpy()

    def step():
        if is_hnsw:
            return step_replicas()
        slot = state["it"] % len(xchs)
        state["it"] += 1
        Ds, Is = Dbuf[slot], Ibuf[slot]
        for q0 in range(gq0, gq1, chunk):
            q1 = min(gq1, q0 + chunk)
            ix.search_torch(xq[q0:q1], ks, D=Ds[q0:q1], I=Is[q0:q1], **search_kw)
        if ip_ties:
            fD, fI = xchs[slot].merge_ip_exact(Ds, Is, xq, lambda xf, T: ix.tie_candidates_torch(xf, T, k))
            if rank == 0:
                final["D"], final["I"] = fD, fI
            return
        if ivf_ties:
            fD, fI = xchs[slot].merge_ivf_exact(metric, Ds, Is, lambda fq, T: ix.ivf_tie_emit_torch(fq, xq, T, k),
                                                        ids_ascending=bool(ix.get_stat("ivf_ids_ascending")))
            if rank == 0:
                final["D"], final["I"] = fD, fI
            return
        if world > 1:
            # exchange step: per-shard (distance,label) blocks over xGMI + copy to pinned host memory, enqueued behind
            # the search; then the host k-way merge (rank 0) -- of the PREVIOUS batch when pipelined, so that it
            # overlaps this batch's search (every merge still happens inside the timed region: fence() drains)
            xchs[slot].gather_async(Ds[gq0:gq1], Is[gq0:gq1])
            if pipelined:
                drain()
                state["pending"] = slot
            else:
                finish(slot)

    def finish(slot):
        fD, fI = xchs[slot].merge_host(metric)
        if rank == 0:
            final["D"], final["I"] = fD, fI

    def drain():
        if state["pending"] is not None:
            finish(state["pending"])
            state["pending"] = None

    def fence():
        drain()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # the FIRST search of an index sizes buffers and learns its data (bucket pitch, filter statistics): timed on its own as the
    # cold step; it is the first of the W warm-up steps, not an extra one
    first_call_ms = None
    for i in range(args.warmup):
        if i == 0:
            fence()
            t_c = time.perf_counter()
            step()
            fence()
            first_call_ms = (time.perf_counter() - t_c) * 1e3
        else:
            step()
    fence()
    ix.set_kernel_timing(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    dt = time.perf_counter() - t0
    ix.set_kernel_timing(False)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    n_launch, kern_ms = ix.kernel_time_stats()
    kinfo = ix.last_kernel_info()

    def _snap(fn):
        try:
            return fn()
        except Exception:  # noqa: BLE001
            return None

    # (the census of the timed searches: the extra searches below must not dilute it)
    snap_collect, snap_prefilter = _snap(ix.collect_stats), _snap(ix.prefilter_stats)
    snap_probe = _snap(ix.ivf_probe_stats) if is_ivf else None  # (of the timed batch, before the extra searches below)
    snap_admitted = _snap(ix.ivf_probe_stats) if not is_ivf and not is_hnsw else None  # (Flat: what the scan admitted in the last search)
    # what the last timed step handed its caller (N > 1: rank 0's merged result, already in `final`), before any search below
    if rank == 0 and world == 1:
        final["D"], final["I"] = D.cpu().numpy(), I.cpu().numpy()
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, final["D"], final["I"])
    # state carried from one search to the next: one batch of DIFFERENT selectivity -- the midpoints of
    # neighbouring queries: nearer the centre of uniform data, between the clusters of clustered data -- then the benchmark's batch
    # again, each timed on its own, outside the timed region
    state_sens = None
    # (under rocprofv3 the extra searches would land in the kernel trace / counter totals of the timed loop: skipped)
    under_profiler = any("rocprof" in os.environ.get(v, "").lower() for v in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "ROCPROFILER_REGISTER_LIBRARY", "HSA_TOOLS_LIB"))
    if args.full and world == 1 and not is_hnsw and chunk == nq and not under_profiler:
        try:
            def one(xx):
                torch.cuda.synchronize()
                t_s = time.perf_counter()
                ix.search_torch(xx, ks, D=D, I=I, **search_kw)
                torch.cuda.synchronize()
                return (time.perf_counter() - t_s) * 1e3

            def cands():
                try:
                    c = ix.collect_stats()
                    return c["candidates"], c["queries"]
                except Exception:  # noqa: BLE001
                    return 0, 0

            def scan():  # (rows the coarse filter admitted in the last search -- before the final-bound filter --, dominant kernel's ms)
                try:
                    adm = ix.ivf_probe_stats()["admitted"] if not is_ivf else None
                    return (round(adm / max(nq, 1), 1) if adm is not None else None), round(ix.last_kernel_info()["last_ms"], 3)
                except Exception:  # noqa: BLE001
                    return None, None

            xq_other = (0.5 * (xq + xq.roll(1, 0))).contiguous()
            if args.normalize:
                xq_other = prep(xq_other)
            # (a search that follows ~50 ms without device work takes ~15 % longer WHATEVER the batch -- clocks and power state of an idle
            # device, profiles/r6_batch_state.txt; the host-side census above is such a gap, so one discarded search comes first and the
            # gap's own cost is reported on its own line.  Round 5's "other batch + 12 %" was this, not the batch.)
            one(xq)
            time.sleep(0.05)
            t_idle = one(xq)
            one(xq)
            c0 = cands()
            t_other = one(xq_other)
            s_other = scan()
            c1 = cands()
            t_after = one(xq)
            s_after = scan()
            c2 = cands()
            t_after2 = one(xq)
            state_sens = {
                "other_batch_admitted_per_query": s_other[0], "step_after_admitted_per_query": s_after[0],
                "step_after_50ms_idle_ms": round(t_idle, 3),
                "first_call_ms": round(first_call_ms, 3) if first_call_ms is not None else None,
                "other_batch": "midpoints of neighbouring queries",
                "other_batch_ms": round(t_other, 3),
                "other_batch_candidates_per_query": round((c1[0] - c0[0]) / max(c1[1] - c0[1], 1), 1),
                "step_after_other_batch_ms": round(t_after, 3),
                "step_after_other_batch_candidates_per_query": round((c2[0] - c1[0]) / max(c2[1] - c1[1], 1), 1),
                "second_step_after_ms": round(t_after2, 3),
                "steady_ms_per_step": round(dt / args.steps * 1e3, 3),
            }
            ix.search_torch(xq, ks, D=D, I=I, **search_kw)  # (D / I hold the benchmark batch's results again)
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            state_sens = {"error": repr(e)[:200]}

    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        qps = nq * args.steps / dt
        out = {
            "metric": "queries/sec, %s %s d=%d N=%d efSearch=%d nq=%d k=%d" % (args.index, args.metric, d, n, args.efsearch, nq, k)
            if is_hnsw
            else "queries/sec, Flat%s d=%d N=%d nq=%d k=%d" % (args.metric, d, n, nq, k)
            if not is_ivf
            else "queries/sec, %s d=%d N=%d nprobe=%d nq=%d k=%d" % (args.index, d, n, args.nprobe, nq, k),
            "value": round(qps, 1),
            "unit": "queries/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak" if is_hnsw else "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic (counter-based %s%s%s, db seed %d, query seed %d)"
            % (
                args.data,
                " centres=%d sigma=%g" % (args.centers, args.sigma) if args.data == "clustered" else "",
                ", rows L2-normalised" if args.normalize else "",
                DB_SEED,
                Q_SEED,
            ),
            "config": {
                "workload": "%s %s d=%d N=%d nq=%d k=%d" % (args.index, args.metric, d, n, nq, k),
                "queries_per_call": chunk,
                "row_shards": 1 if is_hnsw else (args.inlib_shards if args.inlib_shards > 1 else nshards),
                "in_library_shards": (ix.shard_info() or {}).get("devices") if args.inlib_shards > 1 else None,
                "replicas": world if is_hnsw else qgroups,  # (query groups: each holds the whole database as row_shards shards)
                "exchange": (
                    "gather of disjoint result rows"
                    if is_hnsw
                    else "one rccl all_gather of packed {value,label} records + k-way merge on rank 0's device (mvs_merge_records_device)"
                    + (" (the copy-out of batch i overlaps the search of batch i+1)" if pipelined else "")
                )
                if world > 1
                else "none",
                "build_seconds": round(t_build, 2),
                "collective": ranks_seen,
                "state_sensitivity": state_sens,
                "options": args.opt,
                "efConstruction": (args.efconstruction or 40) if is_hnsw else None,
            },
        }
        # achievable HBM bandwidth on THIS box: device-to-device copy of 2 GiB (read + write counted), best of 5
        if args.full:
            try:
                src_t = torch.empty(1 << 29, dtype=torch.float32, device=dev)
                dst_t = torch.empty_like(src_t)
                best = 0.0
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    dst_t.copy_(src_t)
                    e1.record()
                    torch.cuda.synchronize()
                    best = max(best, 2.0 * src_t.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9)
                out["hbm_copy_gbps_measured"] = round(best, 1)
                del src_t, dst_t
            except Exception as e:  # noqa: BLE001
                out["hbm_copy_gbps_measured"] = None
        # ---- roofline of the dominant kernel (per launch, HIP events on the launch stream) ----------
        if n_launch > 0 and kern_ms > 0:
            avg_ms = kern_ms / n_launch
            # HBM bytes per launch come from the committed PMC passes of this same workload (PMC counters cannot be
            # collected from inside the process); null for any other workload
            traffic, traffic_src = None, None
            tname = next((t for t in ("r6_traffic.json", "r5_traffic.json", "r4_traffic.json") if os.path.exists(os.path.join(ROOT, "profiles", t))), "r4_traffic.json")
            tpath = os.path.join(ROOT, "profiles", tname)
            pmc_entry = None
            if os.path.exists(tpath) and world == 1 and chunk == nq and not args.opt and args.efconstruction == 0:
                for w in json.load(open(tpath)).get("workloads", []):
                    # a PMC figure is only valid for the launch it was measured on: same workload, same dominant kernel,
                    # same grid (the planner's split count) -- anything else reports null rather than a stale number
                    if (
                        w["metric"] == out["metric"]
                        and w.get("workload") == out["config"]["workload"]
                        and w["data"] == out["data"]
                        and w.get("kernel") == kinfo["name"]
                        and w.get("grid", kinfo["grid"]) == kinfo["grid"]
                    ):
                        traffic, traffic_src = w["hbm_bytes_per_launch"], "profiles/%s (" % tname + w["source"] + ")"
                        pmc_entry = w
            if kinfo["name"].startswith(("flat_bf16_collect", "flat_bf16_wide", "flat_bf16_big")):
                # bf16 coarse filter (csrc/flat_collect.hip; 128 < d <= 768: csrc/flat_collect_wide.hip): ONE bf16 MFMA product per element pair is the algorithm, so its
                # algorithmic flops are 2 nq N d, priced against the dense bf16 peak; the candidates it admits are re-scored
                # exactly in f32 (their kernels are inside the timed step, not inside this launch)
                st = snap_prefilter
                cs = snap_collect
                achieved = kinfo["flops"] / (avg_ms * 1e-3) / 1e12
                out["dtype"] = "f32 results (bf16 matrix-pipe coarse filter with a proven bound + exact f32 re-scoring of the candidates)"
                out["roofline"] = {
                    "kernel": kinfo["name"],
                    "bound": "mfma",
                    "achieved": round(achieved, 1),
                    "peak": PEAK_BF16_MFMA_TFLOPS,
                    "unit": "TFLOP/s",
                    "frac": round(achieved / PEAK_BF16_MFMA_TFLOPS, 4),
                    "traffic": traffic,
                    "traffic_source": traffic_src,
                    "avg_launch_ms": round(avg_ms, 4),
                    "launches": n_launch,
                    "algorithmic_flops_per_launch": kinfo["flops"],
                    "f32_equivalent_vs_f32_mfma_peak": round(achieved / PEAK_F32_MFMA_TFLOPS, 3),
                    "algorithmic_bytes_per_launch": kinfo["bytes"],
                    "hbm_frac_of_8TBps": round(kinfo["bytes"] / (avg_ms * 1e-3) / 1e9 / PEAK_HBM_GBPS, 5),
                    "grid": kinfo["grid"],
                    "lds_bytes": kinfo["lds_bytes"],
                    "candidates_rescored_per_query": round(cs["candidates"] / max(cs["queries"], 1), 1),
                    "candidates_admitted_per_query": (round(snap_admitted["admitted"] / max(nq, 1), 1) if snap_admitted else None),
                    "candidate_stream_overflows": cs["overflows"],
                    "queries_rerun_on_exact_kernel": st["fallback_queries"],
                }
            elif kinfo["name"].startswith("flat_bf16x3"):
                # bf16x3 prefilter (csrc/flat_bf16.hip): three bf16 MFMA products per element pair are the algorithm
                # (hi*hi + hi*lo + lo*hi), so its algorithmic flops are 3 x 2 nq N d, priced against the dense bf16 peak
                st = snap_prefilter
                exec_flops = 3.0 * kinfo["flops"]
                achieved = exec_flops / (avg_ms * 1e-3) / 1e12
                out["dtype"] = "f32 results (bf16x3 matrix-pipe prefilter + exact f32 re-scoring of the candidates)"
                out["roofline"] = {
                    "kernel": kinfo["name"],
                    "bound": "mfma",
                    "achieved": round(achieved, 1),
                    "peak": PEAK_BF16_MFMA_TFLOPS,
                    "unit": "TFLOP/s",
                    "frac": round(achieved / PEAK_BF16_MFMA_TFLOPS, 4),
                    "traffic": traffic,
                    "traffic_source": traffic_src,
                    "avg_launch_ms": round(avg_ms, 4),
                    "launches": n_launch,
                    "algorithmic_flops_per_launch": exec_flops,
                    "f32_equivalent_tflops": round(kinfo["flops"] / (avg_ms * 1e-3) / 1e12, 1),
                    "f32_equivalent_vs_f32_mfma_peak": round(kinfo["flops"] / (avg_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 3),
                    "algorithmic_bytes_per_launch": kinfo["bytes"],
                    "hbm_frac_of_8TBps": round(kinfo["bytes"] / (avg_ms * 1e-3) / 1e9 / PEAK_HBM_GBPS, 5),
                    "grid": kinfo["grid"],
                    "lds_bytes": kinfo["lds_bytes"],
                    "queries_rerun_on_exact_kernel": st["fallback_queries"],
                    "queries_served": st["queries"],
                    "observed_max_rel_err": st["max_rel_err"],
                    "proof_err_bound": st["err_bound"],
                }
            elif kinfo["name"].startswith("flat_mfma"):
                achieved = kinfo["flops"] / (avg_ms * 1e-3) / 1e12
                out["roofline"] = {
                    "kernel": kinfo["name"],
                    "bound": "mfma",
                    "achieved": round(achieved, 2),
                    "peak": PEAK_F32_MFMA_TFLOPS,
                    "unit": "TFLOP/s",
                    "frac": round(achieved / PEAK_F32_MFMA_TFLOPS, 4),
                    "traffic": traffic,
                    "traffic_source": traffic_src,
                    "avg_launch_ms": round(avg_ms, 4),
                    "launches": n_launch,
                    "algorithmic_flops_per_launch": kinfo["flops"],
                    "algorithmic_bytes_per_launch": kinfo["bytes"],
                    "hbm_frac_of_8TBps": round(kinfo["bytes"] / (avg_ms * 1e-3) / 1e9 / PEAK_HBM_GBPS, 5),
                    "grid": kinfo["grid"],
                    "lds_bytes": kinfo["lds_bytes"],
                }
            else:
                achieved = kinfo["bytes"] / (avg_ms * 1e-3) / 1e9
                out["roofline_note"] = (
                    "achieved = distance evaluations counted by the kernel x (4d + 4) bytes / launch time (SURVEY 8d C5)"
                    if is_hnsw
                    else "achieved = list-major algorithmic bytes (every work item streams its list once) / launch time"
                )
                out["roofline"] = {
                    "kernel": kinfo["name"],
                    "bound": "hbm",
                    "achieved": round(achieved, 1),
                    "peak": PEAK_HBM_GBPS,
                    "unit": "GB/s",
                    "frac": round(achieved / PEAK_HBM_GBPS, 4),
                    "traffic": traffic,
                    "traffic_source": traffic_src,
                    "avg_launch_ms": round(avg_ms, 4),
                    "launches": n_launch,
                    "algorithmic_bytes_per_launch": kinfo["bytes"],
                    "traffic_over_algorithmic": round(traffic / kinfo["bytes"], 3) if traffic else None,
                    "grid": kinfo["grid"],
                }
                if is_hnsw:
                    # what the walk actually pulls out of the row stores per launch: a bf16 row (2d bytes) for every neighbour
                    # looked at first, an f32 row (4d) for those that could still matter -- against the ALGORITHMIC 4d + 4 per
                    # evaluation above (what FAISS's walk reads, the unit of SURVEY 8d)
                    try:
                        ws = ix.hnsw_walk_stats()
                        moved = ws["bf16_rows"] * 2.0 * d + ws["f32_rows"] * 4.0 * d
                        out["roofline"]["row_bytes_moved_per_launch"] = moved
                        out["roofline"]["row_bytes_moved_GBps"] = round(moved / (avg_ms * 1e-3) / 1e9, 1)
                        out["roofline"]["f32_rows_fetched_frac"] = round(ws["f32_rows"] / max(ws["evaluations"], 1.0), 4)
                    except Exception as e:  # noqa: BLE001
                        out["roofline"]["row_bytes_moved_per_launch"] = None
                        out["roofline_moved_error"] = str(e)[:200]
                if is_ivf:
                    # SURVEY 8d's own figure: every stored vector and id read ONCE per batch (list-major lower bound),
                    # whatever the number of <= 20-query work items that actually stream a list
                    # (an f32 figure the bf16 kernel never moves: reported as bytes only, not as a bandwidth -- VERDICT r4 #6)
                    lm = float(n) * d * 4 + float(n) * 8
                    out["roofline"]["list_major_bytes_8d"] = lm
                    try:  # census of the IVF coarse filter (csrc/ivf_collect.hip): candidates re-scored exactly, per query
                        cs = snap_collect
                        out["roofline"]["candidates_rescored_per_query"] = round(cs["candidates"] / max(cs["queries"], 1), 1)
                    except Exception:  # noqa: BLE001
                        pass
                    try:  # probe pruning (csrc/ivf_collect.hip ivf_probe_prune_kernel): (query, list) pairs asked for / scanned
                        ps = snap_probe
                        out["roofline"]["probe_pairs"] = ps["pairs"]
                        out["roofline"]["probe_pairs_scanned"] = ps["scanned"]
                        out["roofline"]["scan_forced_drains"] = ps["forced_drains"]
                        out["roofline"]["candidates_admitted_per_query"] = round(ps["admitted"] / max(nq, 1), 1)
                        out["roofline"]["probe_pruning_note"] = ("probed lists that provably hold none of a query's k nearest rows (triangle "
                                                                 "inequality on coarse distance and list radius) are not scanned; labels and "
                                                                 "distances are those of scanning all nprobe lists (parity_device / the oracle)")
                    except Exception:  # noqa: BLE001
                        pass
        # ---- CPU baseline (oracle, BLAS-path arithmetic, all host cores) + recall, N=1 only ----------
        if world == 1 and is_hnsw:
            out["distance_evals_per_query"] = round(kinfo["bytes"] / (4.0 * d + 4.0) / nq, 1)
            out["expanded_vertices_per_query"] = kinfo["nsplit"]
        if args.full and world == 1 and is_hnsw:
            ns = min(nq, 1000)
            flat = mf.index_factory(d, "Flat", metric)
            for s0 in range(0, n, 1 << 20):
                m = min(1 << 20, n - s0)
                flat.add_torch(prep(gen(m, d, DB_SEED, row0=s0, device=dev)))
            _, Igt = flat.search_torch(xq[:ns].contiguous(), k)
            torch.cuda.synchronize()
            Igt = Igt.cpu().numpy()
            out["recall_at_10"] = round(
                float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(final["I"][:ns], Igt)])), 5
            )
            out["recall_sample_queries"] = ns
            if args.efconstruction == 0 and not args.opt:
                # FAISS's default efConstruction = 40 is what the reference's harness builds (its 'efConstruct' key is ignored,
                # SURVEY Appendix C) and what `value` is measured on; the same workload on an efConstruction = 200 graph, as a
                # secondary entry: recall and QPS of the walk when the graph is built the way one would for serving
                try:
                    ix2 = mf.index_factory(d, args.index, metric)
                    ix2.set_ef_construction(200)
                    tb0 = time.time()
                    for s0 in range(0, n, 1 << 16):
                        m = min(1 << 16, n - s0)
                        xb2 = prep(gen(m, d, DB_SEED, row0=s0, device=dev))
                        ix2.add_torch(xb2, ids=torch.arange(s0, s0 + m, dtype=torch.int64, device=dev) if with_ids else None)
                        torch.cuda.synchronize()
                    tb = time.time() - tb0
                    D2, I2 = torch.empty_like(D), torch.empty_like(I)
                    ix2.search_torch(xq, k, D=D2, I=I2, **search_kw)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    for _ in range(args.steps):
                        ix2.search_torch(xq, k, D=D2, I=I2, **search_kw)
                    torch.cuda.synchronize()
                    t2 = (time.perf_counter() - t1) / args.steps
                    I2h = I2[:ns].cpu().numpy()
                    out["recall_efConstruction_200"] = {
                        "recall_at_10": round(float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(I2h, Igt)])), 5),
                        "value": round(nq / t2, 1), "unit": "queries/s", "ms_per_step": round(t2 * 1e3, 3), "build_seconds": round(tb, 2),
                    }
                    del ix2, D2, I2
                except Exception as e:  # noqa: BLE001
                    out["recall_efConstruction_200"] = {"error": repr(e)[:200]}
            if not args.no_cpu_baseline:
                from oracle import oracle as orc

                # the oracle walks the SAME graph (a single-thread oracle build of N rows would take hours):
                # rows come back from the device generator, the graph from the device index
                xb_h = np.empty((n, d), dtype=np.float32)
                for s0 in range(0, n, 1 << 20):
                    m = min(1 << 20, n - s0)
                    xb_h[s0 : s0 + m] = prep(gen(m, d, DB_SEED, row0=s0, device=dev)).cpu().numpy()
                del flat
                o = orc.Index(d, args.index.replace("IDMap,", ""), metric)
                o.hnsw_set_graph(xb_h, ix.hnsw_graph())
                xq_h = xq.cpu().numpy()
                nq_cpu, done, t_cpu = 256, 0, 0.0
                same = True
                ref_parts = []
                while t_cpu < args.cpu_seconds and done < nq:
                    m = min(nq_cpu, nq - done)
                    t1 = time.perf_counter()
                    Do, Io = o.search(xq_h[done : done + m], k, efSearch=args.efsearch)
                    t_cpu += time.perf_counter() - t1
                    same &= bool(np.array_equal(final["I"][done : done + m], Io))
                    same &= bool(np.array_equal(final["D"][done : done + m].view(np.uint32), Do.view(np.uint32)))
                    ref_parts.append((Do, Io))
                    done += m
                    nq_cpu = min(4096, nq_cpu * 2)
                # The walk's MinimaxHeap::pop_min takes, of several EQUAL minima, the one that sits last in FAISS's heap array; the
                # device walk takes the smallest id.  The oracle has both rules: how many of the sampled queries
                # change ANY label or distance between them on this data?  (a deviation documented by measurement)
                try:
                    orc.hnsw_set_pop_min_rule(1)
                    differ, pos = 0, 0
                    for Do, Io in ref_parts:
                        m = len(Io)
                        D1, I1 = o.search(xq_h[pos : pos + m], k, efSearch=args.efsearch)
                        differ += int(((I1 != Io).any(axis=1) | (D1.view(np.uint32) != Do.view(np.uint32)).any(axis=1)).sum())
                        pos += m
                    out["hnsw_pop_min_tie_rule"] = {"queries": done, "results_differ_between_array_order_and_id_order": differ}
                finally:
                    orc.hnsw_set_pop_min_rule(0)
                out["cpu_baseline"] = {
                    "value": round(done / t_cpu, 2),
                    "unit": "queries/s",
                    "cores": orc.num_threads(),
                    "kind": "port",
                    "sample": "%d of %d queries, efSearch=%d, on the device-built graph (oracle/orc_hnsw.c "
                    "orc_hnsw_search_one, OpenMP over queries) in %.1f s" % (done, nq, args.efsearch, t_cpu),
                }
                out["labels_and_distances_bit_exact_vs_oracle"] = same
        if args.full and world == 1 and is_ivf:
            # recall@10 against exact Flat ground truth (the Flat path is bit-exact vs the oracle) on a query sample
            ns = min(nq, 1000)
            flat = mf.index_factory(d, "Flat", metric)
            for s0 in range(0, n, slab):
                flat.add_torch(xb_all[s0 : s0 + slab])
            _, Igt = flat.search_torch(xq[:ns].contiguous(), k)
            torch.cuda.synchronize()
            Igt = Igt.cpu().numpy()
            out["recall_at_10"] = round(
                float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(final["I"][:ns], Igt)])), 5
            )
            out["recall_sample_queries"] = ns
            del flat
            if not args.no_cpu_baseline:
                from oracle import oracle as orc

                xb_h = xb_all.cpu().numpy()
                xq_h = xq.cpu().numpy()
                o = orc.Index(d, args.index, metric)
                o.ivf_set_centroids(ix.ivf_centroids())  # share the trained centroids; time add separately from search
                t1 = time.perf_counter()
                o.add(xb_h)
                t_add = time.perf_counter() - t1
                nq_cpu = min(nq, 2048)
                t1 = time.perf_counter()
                Do, Io = o.search(xq_h[:nq_cpu], k, nprobe=args.nprobe)
                t_cpu = time.perf_counter() - t1
                same = np.array([len(np.unique(r)) == k for r in Do])
                out["cpu_baseline"] = {
                    "value": round(nq_cpu / t_cpu, 2),
                    "unit": "queries/s",
                    "cores": orc.num_threads(),
                    "kind": "port",
                    "sample": "%d of %d queries, nprobe=%d, index shares the device-trained centroids; oracle add of N=%d "
                    "took %.1f s (oracle/orc_core.c ivf_search, OpenMP over queries)" % (nq_cpu, nq, args.nprobe, n, t_add),
                }
                out["labels_bit_exact_vs_oracle"] = bool(np.array_equal(final["I"][:nq_cpu][same], Io[same]))
        if args.full and world == 1 and not args.no_cpu_baseline and not is_ivf and not is_hnsw:
            from oracle import oracle as orc

            xb_h = host_rows(n, DB_SEED)
            xq_h = xq.cpu().numpy()
            cores = orc.num_threads()
            # (a) cpu_baseline = FAISS's BLAS branch on the REAL OpenBLAS (oracle/orc_core.c search_openblas: FAISS's 4096 x 1024
            # blocking, norms formula, heaps; sgemm from numpy's bundled OpenBLAS 0.3.29 = the reference's vcpkg pin) on a bounded
            # query sample against the full database -- the CPU path north_star names, and the INDEPENDENT label reference:
            # sgemm sums in its own order, so the census below counts the (query, rank) slots that differ from the device and
            # checks that each sits inside the rounding band.  Searched at k + 1 so the gap behind the last slot is known.
            half = args.cpu_seconds / 2.0
            try:
                ob_cfg = orc.openblas_load()
                # FAISS hands sgemm 4096-query x 1024-row blocks (1 GFLOP at d = 128): small for a thread pool.  Measured on the GPU
                # box's host (256 hardware threads; profiles/r4_openblas_threads.txt): 64 OpenBLAS threads 81 q/s, 32: 162, 16: 244,
                # 8: 250 at the headline shape with 4096-query blocks; 1024-query blocks lose another 2.5x.  So: 16 threads, and
                # whole 4096-query blocks whenever the budget allows.
                # (round 5, ADVICE r4: not hard-coded -- a short probe on this host picks among 8 / 16 / 32, the sweep is in the line)
                ob_threads, ob_sweep = min(16, os.cpu_count() or 16), {}
                try:
                    pr, pq = min(n, 1 << 18), min(nq, 4096)
                    for t_try in (8, 16, 32):
                        if t_try > (os.cpu_count() or 16):
                            continue
                        orc.openblas_set_num_threads(t_try)
                        t1 = time.perf_counter()
                        orc.flat_search(metric, xb_h[:pr], xq_h[:pq], k + 1, force_path=orc.PATH_OPENBLAS)
                        ob_sweep[t_try] = round(pq / (time.perf_counter() - t1) * pr / n, 1)  # queries/s scaled to the full N
                    if ob_sweep:
                        ob_threads = max(ob_sweep, key=ob_sweep.get)
                except Exception:  # noqa: BLE001
                    pass
                orc.openblas_set_num_threads(ob_threads)
                est = 2.0 * 4096 * n * d / 0.6e12
                nq_ob = min(nq, 4096 if est <= 1.3 * half else (1024 if est <= 5 * half else max(64, int(1024 * 4 * half / est) // 64 * 64)))
                t_ob, done_ob = 0.0, 0
                refD, refI = [], []
                while done_ob < nq and (done_ob == 0 or t_ob + t_ob / done_ob * nq_ob <= half):
                    m = min(nq_ob, nq - done_ob)
                    t1 = time.perf_counter()
                    Dr, Ir = orc.flat_search(metric, xb_h, xq_h[done_ob : done_ob + m], k + 1, force_path=orc.PATH_OPENBLAS)
                    t_ob += time.perf_counter() - t1
                    refD.append(Dr), refI.append(Ir)
                    done_ob += m
                refD, refI = np.concatenate(refD), np.concatenate(refI)
                out["cpu_baseline"] = {
                    "value": round(done_ob / t_ob, 2),
                    "unit": "queries/s",
                    "cores": ob_threads,
                    "cores_note": "%d OpenBLAS threads in sgemm (picked by a probe on this host: queries/s scaled to N per thread count = %s), %d OpenMP threads in the norms / heap loops" % (ob_threads, ob_sweep, cores),
                    "thread_sweep_qps": ob_sweep,
                    "kind": "openblas",
                    # (say what this baseline is next to the number)
                    "note": "a weak CPU baseline: the fastest of 1..%d OpenBLAS threads on a shared %d-thread host (its sgemm peaks near 2 TFLOP/s here) -- reported, not the target" % (max(ob_threads, 16), os.cpu_count() or 0),
                    "sample": "%d of %d queries vs the full N=%d database in %.1f s: FAISS's BLAS branch (4096 x 1024 sgemm blocks, "
                    "(xn+yn)-2ip, CMax/CMin heaps at k+1=%d) on %s" % (done_ob, nq, n, t_ob, k + 1, ob_cfg),
                }
                cen = orc.openblas_census(metric, xb_h, xq_h[:done_ob], k, final["D"][:done_ob], final["I"][:done_ob], ref=(refD, refI))
                out["labels_equal_vs_openblas"] = cen["slots_label_differs"] == 0
                out["openblas_census"] = cen
            except Exception as e:  # noqa: BLE001  (no OpenBLAS on the host: the port below is the baseline)
                out["openblas_error"] = repr(e)[:300]
            # (b) the oracle's own BLAS-branch restatement (k-ordered fma chain = what the device computes bit for bit): the
            # bit-exact label check, and the baseline when no OpenBLAS exists
            est = 2.0 * 4096 * n * d / 0.5e12
            nq_cpu = 4096 if est <= 2 * half else max(256, int(4096 * 2 * half / est) // 256 * 256)
            t_cpu, done = 0.0, 0
            hits = total = 0
            labels_equal = True
            while t_cpu < half and done < nq:
                m = min(nq_cpu, nq - done)
                t1 = time.perf_counter()
                Do, Io = orc.flat_search(metric, xb_h, xq_h[done : done + m], k, force_path=orc.PATH_BLAS)
                step_t = time.perf_counter() - t1
                t_cpu += step_t
                g = final["I"][done : done + m]
                labels_equal &= bool(np.array_equal(g, Io))
                for a, b in zip(g, Io):
                    hits += len(set(a.tolist()) & set(b.tolist()))
                    total += k
                done += m
                per_q = t_cpu / done
                nq_cpu = int(max(24, min(4096, (half - t_cpu) / max(per_q, 1e-9))))
                if half - t_cpu < per_q * 24:
                    break
            port = {
                "value": round(done / t_cpu, 2),
                "unit": "queries/s",
                "cores": cores,
                "kind": "port",
                "sample": "%d of %d queries vs the full N=%d database in %.1f s (oracle/orc_core.c search_blas: "
                "packed AVX2 k-ordered-fma GEMM + heaps, OpenMP)" % (done, nq, n, t_cpu),
            }
            # both baselines under explicit names; `cpu_baseline` (the contract's key) = the FASTER of the two, so that a speed-up
            # computed from it is the conservative one
            out["cpu_baseline_port"] = port
            if "cpu_baseline" in out:
                out["cpu_baseline_openblas"] = out["cpu_baseline"]
                if port["value"] > out["cpu_baseline"]["value"]:
                    out["cpu_baseline"] = dict(port)
                out["cpu_baseline"] = dict(out["cpu_baseline"], selected="max(cpu_baseline_openblas, cpu_baseline_port) by value")
            else:
                out["cpu_baseline"] = dict(port, selected="cpu_baseline_port (no OpenBLAS on this host)")
            out["recall_at_10"] = round(hits / max(total, 1), 6)
            out["labels_bit_exact_vs_oracle"] = labels_equal
            out["recall_sample_queries"] = done
            # second CPU number: the sgemm that dominates CPU FAISS's BLAS branch, alone, on OpenBLAS (numpy, all host
            # threads) -- an UPPER bound for a CPU FAISS+OpenBLAS search (norms, formula and heap updates excluded).
            # Not a parity reference (sgemm's summation order is its own); bounded to a few seconds.
            try:
                qb = np.ascontiguousarray(xq_h[: min(nq, 2048)])
                _ = qb @ xb_h[: 1 << 16].T  # warm the thread pool
                t_gemm, rows_done = 0.0, 0
                for r0 in range(0, n, 1 << 18):
                    blk = xb_h[r0 : r0 + (1 << 18)]
                    t1 = time.perf_counter()
                    ip = qb @ blk.T
                    t_gemm += time.perf_counter() - t1
                    rows_done += len(blk)
                    del ip
                    if t_gemm > max(3.0, args.cpu_seconds / 3):
                        break
                tf = 2.0 * len(qb) * rows_done * d / t_gemm / 1e12
                out["cpu_sgemm_upper_bound"] = {
                    "value": round(len(qb) / (t_gemm * n / rows_done), 2),
                    "unit": "queries/s",
                    "tflops": round(tf, 3),
                    "kind": "numpy/OpenBLAS sgemm only (%d queries x %d of %d rows timed, scaled to N); norms, distance "
                    "formula and top-k excluded" % (len(qb), rows_done, n),
                }
            except Exception as e:  # noqa: BLE001  (never let the extra number break the bench line)
                out["cpu_sgemm_upper_bound"] = {"error": repr(e)[:200]}
        if args.full and world > 1 and not args.no_cpu_baseline and not is_ivf and not is_hnsw:
            # N > 1: no CPU timing, but the MERGED result of the row shards is checked against the oracle's search of
            # the whole database on a query sample (outside the timed region)
            try:
                from oracle import oracle as orc

                ns = min(nq, 256)
                xb_h, xq_h = host_rows(n, DB_SEED), xq[:ns].cpu().numpy()
                Do, Io = orc.flat_search(metric, xb_h, xq_h, k, force_path=orc.PATH_BLAS)
                out["merged_labels_bit_exact_vs_oracle"] = bool(np.array_equal(final["I"][:ns], Io))
                out["merged_distances_bit_exact_vs_oracle"] = bool(
                    np.array_equal(final["D"][:ns].view(np.uint32), Do.view(np.uint32))
                )
                out["recall_at_10"] = round(
                    float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(final["I"][:ns], Io)])), 6
                )
                out["recall_sample_queries"] = ns
            except Exception as e:  # noqa: BLE001  (the check must never cost the scaling run its bench line)
                out["merged_check_error"] = repr(e)[:200]
        if "roofline" in out and n_launch > 0 and kern_ms > 0:
            r_ = out["roofline"]
            r_["traffic_note"] = ("constant from the committed PMC passes of this workload (counters cannot be read from inside the "
                                  "process), not a measurement of this run") if r_.get("traffic") else None
            if r_.get("traffic"):
                # what the counters say the memory side moved, over THIS run's launch time (beside the algorithmic `frac`)
                r_["frac_counter"] = round(r_["traffic"] / (kern_ms / n_launch * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4)
            if pmc_entry and pmc_entry.get("mfma_busy_frac") is not None:
                r_["mfma_busy_frac"] = pmc_entry["mfma_busy_frac"]
                r_["mfma_busy_source"] = pmc_entry.get("mfma_busy_source")
        if "roofline" in out:
            # the same algorithmic work over the WHOLE step (every kernel of the search, launch gaps included)
            out["roofline"]["frac_step"] = round(out["roofline"]["frac"] * (kern_ms / n_launch) * (n_launch / args.steps) / ms_per_step, 4)
        if world == 1 and args.parity_device > 0 and not is_hnsw:
            ns = min(nq, args.parity_device)
            ix.set_option("ivf_collect" if is_ivf else "prefilter", 0)
            De, Ie = ix.search_torch(xq[:ns].contiguous(), k, **search_kw)
            torch.cuda.synchronize()
            ix.set_option("ivf_collect" if is_ivf else "prefilter", -1)
            out["parity_device"] = {
                "against": ("ivf_scan_kernel (scanner arithmetic)" if is_ivf else "flat_mfma_resident_kernel (exact f32)")
                + ", itself bit-exact vs the oracle in tests/test_configs_gpu.py",
                "kernel": ix.last_kernel_info()["name"],
                "queries": ns,
                "labels_equal": bool(np.array_equal(final["I"][:ns], Ie.cpu().numpy())),
                "distances_bit_equal": bool(np.array_equal(final["D"][:ns].view(np.uint32), De.cpu().numpy().view(np.uint32))),
            }
        headline_default = (
            args.full and world == 1 and args.index == "Flat" and n == 10_000_000 and d == 128 and nq == 10_000 and k == 10
            and args.metric == "L2" and chunk == nq and not args.opt and args.data == "uniform" and not args.normalize
        )
        # under rocprofv3 the extra searches and child processes would land in the kernel trace / counter totals (and the children
        # would be started from a process whose GPU the profiler's preload already initialised): the profiled run is the timed loop only
        profiled = any("rocprof" in os.environ.get(v, "").lower() for v in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "ROCPROFILER_REGISTER_LIBRARY", "HSA_TOOLS_LIB"))
        if profiled:
            out["profiler_detected"] = "embedded configs and host-pointer timing skipped"
            headline_default = False
        if headline_default and not args.no_host_pointer:
            out["host_pointer"] = host_pointer_timing(ix, xq, k, np, time)
        if headline_default and not args.no_configs:
            del ix, xq, D, I
            torch.cuda.empty_cache()
        if headline_default and not args.no_ingest and not args.no_configs:  # (--no-configs = no extras at all)
            out["ingest"] = ingest_lines()
        if headline_default and not args.no_configs:
            out["configs"] = embedded_configs()
    if world > 1:
        # every rank lets go of its GPU before rank 0 starts the secondary layouts as child launches on the same devices
        want_secondary = (args.secondary and not args.no_secondary and args.index == "Flat" and chunk == nq and not args.opt and qgroups == 1)
        ix = xq = D = I = Dbuf = Ibuf = xchs = None
        torch.cuda.empty_cache()
        dist.barrier()
        dist.destroy_process_group()
        if rank == 0 and want_secondary:
            # the measured headline is on disk before any child starts (a kill in the window below loses the extras, not the number)
            try:
                os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
                with open(os.path.join(ROOT, "gpurun_out", "bench_headline_last.json"), "w") as f:
                    f.write(json.dumps(out) + "\n")
            except OSError:
                pass
            out["secondary"] = secondary_layouts(args, world)
    if rank == 0:
        print(json.dumps(compact_line(out)), flush=True)


if __name__ == "__main__":
    main()
