"""CPU-side checks of the pre-transform boundary: the header declares the kind, the functions and the contract's key phrases, the built
library exports the functions, the Python host lists them, the tests' own "IxPT" writer and parser agree with each other, the CPU model's
PCA recovers a planted spectrum, and the apply kernel compiles without scratch."""
import ctypes
import os
import re

import numpy as np

import pretransform_reference as ptr
import refine_reference as rfr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_faiss.h")
FUNCTIONS = {"mvs_index_pretransform_sub": r"mvs_index\s*\*", "mvs_index_pretransform_count": "int", "mvs_index_pretransform_info": "int",
             "mvs_index_pretransform_get_linear": "int", "mvs_index_pretransform_set_linear": "int", "mvs_index_pretransform_get_pca": "int",
             "mvs_index_pretransform_apply": "int", "mvs_index_pretransform_apply_device": "int"}


def test_header_declares_the_pretransform_kind_functions_and_contract():
    full = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert re.search(r"#define\s+MVS_KIND_PRETRANSFORM\s+11\b", src)
    for name, v in (("MVS_VT_LINEAR", 0), ("MVS_VT_PCA", 1), ("MVS_VT_NORM", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, v), src), name
    for name, ret in FUNCTIONS.items():
        assert re.search(r"%s\s*%s\s*\(" % (ret, name), src), name
    for phrase in ("IxPT", "IDMap(PreTransform(sub))", "PCA<o>", "PCAW<o>", "L2norm", "1 <= o <= d_in <= 2048", "PCAR<o>", "PCAWR<o>", "RR<o>", "ITQ<o>",
                   "Pad<o>", "LDA<o>", "acc = fmaf(x[k], A[j][k], acc), k ascending from +0", "ONE f32 addition after the chain",
                   "absent without a bias", "v_mfma_f32_32x32x2_f32", "acc = fmaf(x[k], x[k], acc) from +0", "inv = 1.0f / sqrtf(nr)",
                   "fvec_renorm_L2", "Only norm 2", "no floating-point atomics", "<= 1e-12", "at most 30 sweeps", "DEPARTURE",
                   "rounded once to f32", "(lambda_i + epsilon)^(-1/2)", "accumulated in f64 over the f32 values with k ascending",
                   "n < d_out fails", "already trained is\n *             left alone", "within 256 MB", "'is_trained'", "RESTATED FROM MEMORY",
                   "\"PcAm\"", "\"PCAm\"", "\"VNrm\"", "\"LTra\"", "\"rrot\"", "refused by name", "pretransform_apply_launches",
                   "pretransform_workspace_bytes", "This index type is not implemented\"", "could not parse index string"):
        assert phrase in full, phrase


def test_library_exports_the_pretransform_functions():
    import mi355_faiss as mf

    L = ctypes.CDLL(mf.LIB_PATH)
    missing = [n for n in FUNCTIONS if not hasattr(L, n)]
    assert not missing, missing


def test_python_host_lists_the_pretransform_functions():
    import mi355_faiss as mf

    assert mf.KIND_PRETRANSFORM == 11 and (mf.VT_LINEAR, mf.VT_PCA, mf.VT_NORM) == (0, 1, 2)
    for name in FUNCTIONS:
        assert name in mf.DECLARED_SYMBOLS, name
    for prop in ("pretransform_sub", "pretransform_count"):
        assert isinstance(getattr(mf.Index, prop), property), prop
    for meth in ("pretransform_info", "pretransform_get_linear", "pretransform_set_linear", "pretransform_get_pca", "pretransform_apply",
                 "pretransform_apply_torch"):
        assert callable(getattr(mf.Index, meth)), meth


def test_ixpt_image_round_trips_through_the_python_writer_and_parser():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((3, 5)).astype(np.float32)
    b = rng.standard_normal(3).astype(np.float32)
    pca = dict(fourcc=b"PcAm", d_in=5, d_out=3, A=A, b=b, eigen_power=-0.5, epsilon=0.0, random_rotation=False, balanced_bins=0,
               mean=rng.standard_normal(5), eigenvalues=np.arange(5, 0, -1), PCAMat=rng.standard_normal((5, 5)))
    old = dict(pca, fourcc=b"PCAm")
    chain = [dict(fourcc=b"VNrm", d_in=5, d_out=5, norm=2.0), pca, dict(fourcc=b"LTra", d_in=3, d_out=3, A=np.eye(3), b=None),
             dict(fourcc=b"rrot", d_in=3, d_out=3, A=np.eye(3)[::-1], b=None)]
    rows = rng.standard_normal((7, 3)).astype(np.float32)
    sub = rfr.flat_image(3, ptr.L2, rows)
    for id_map in (None, np.arange(7, dtype=np.int64) * 5 + 2):
        buf = ptr.write_pretransform(None, 5, ptr.L2, chain, sub, ntotal=7, id_map=id_map)
        assert buf[:4] == (b"IxPT" if id_map is None else b"IxMp")
        img = ptr.parse_pretransform(buf)
        assert (img["d"], img["ntotal"], img["trained"], img["metric"]) == (5, 7, True, ptr.L2)
        assert img["sub"] == sub and [t["fourcc"] for t in img["chain"]] == [b"VNrm", b"PcAm", b"LTra", b"rrot"]
        assert (img["id_map"] is None) if id_map is None else np.array_equal(img["id_map"], id_map)
        n, p, l, r = img["chain"]
        assert n["type"] == ptr.VT_NORM and n["norm"] == 2.0 and (n["d_in"], n["d_out"]) == (5, 5)
        assert p["type"] == ptr.VT_PCA and p["have_bias"] and p["eigen_power"] == -0.5 and p["epsilon"] == 0.0 and p["balanced_bins"] == 0
        assert np.array_equal(p["A"], A) and np.array_equal(p["b"], b) and p["mean"].size == 5 and p["PCAMat"].size == 25
        assert l["type"] == ptr.VT_LINEAR and not l["have_bias"] and l["b"].size == 0 and np.array_equal(l["A"], np.eye(3, dtype=np.float32))
        assert r["is_trained"] and np.array_equal(r["A"], np.eye(3, dtype=np.float32)[::-1])
    # the old PCA fourcc lacks epsilon: four bytes shorter, everything else equal
    assert len(ptr.transform_bytes(old)) + 4 == len(ptr.transform_bytes(pca))
    assert ptr.parse_pretransform(ptr.write_pretransform(None, 5, ptr.L2, [old], sub))["chain"][0]["eigen_power"] == -0.5
    # the layout of one plain transform: fourcc, have_bias, u64 count + A, u64 count + b, d_in, d_out, is_trained -- nothing else
    t = ptr.transform_bytes(dict(fourcc=b"LTra", d_in=2, d_out=1, A=[[1.0, 2.0]], b=[3.0]))
    assert t == b"LTra" + b"\x01" + (2).to_bytes(8, "little") + np.float32([1, 2]).tobytes() + (1).to_bytes(8, "little") + np.float32([3]).tobytes() + \
        (2).to_bytes(4, "little") + (1).to_bytes(4, "little") + b"\x01"


def test_model_pca_recovers_the_planted_spectrum():
    x = ptr.planted()
    m = ptr.pca_train(x, 5)
    rel, ab = ptr.spectrum_gaps(m["lam64"])
    assert rel >= 0.25 and ab >= 1e-4, (rel, ab)
    assert np.allclose(m["lam64"], 2.0 ** -np.arange(12), rtol=0.1)  # (n = 4096 samples: a few per cent of sampling error)
    V = m["V64"]
    assert np.abs(V @ V.T - np.eye(12)).max() < 1e-12
    assert np.abs(V @ m["C"] @ V.T - np.diag(m["lam64"])).max() < 1e-12
    assert all(v[np.argmax(np.abs(v))] > 0 for v in V)
    assert m["A"].shape == (5, 12) and np.array_equal(m["A"], m["PCAMat"][:5])
    # the bias centres the data: the transformed rows have zero mean to f32 accuracy
    y = x.astype(np.float64) @ m["A"].astype(np.float64).T + m["b"].astype(np.float64)
    assert np.abs(y.mean(axis=0)).max() < 1e-5
    w = ptr.pca_train(x, 5, whiten=True)
    yw = x.astype(np.float64) @ w["A"].astype(np.float64).T + w["b"].astype(np.float64)
    assert np.abs(yw.var(axis=0) - 1.0).max() < 1e-4
    # the bias rule by hand: b = -(A mean), products exact in f64
    assert ptr.pca_bias([[1.0, 2.0], [0.5, -4.0]], [3.0, 0.25]).tolist() == [-3.5, -0.5]


def test_model_linear_and_l2norm_by_hand():
    A = np.array([[1.0, 2.0, 3.0], [0.0, -1.0, 0.5]], dtype=np.float32)
    x = np.array([[1.0, 1.0, 1.0], [2.0, 0.0, -2.0], [np.nan, 1.0, 1.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    y = ptr.linear(A, [10.0, 20.0], x)
    assert y[0].tolist() == [16.0, 19.5] and y[1].tolist() == [6.0, 19.0] and np.isnan(y[2]).all() and y[3].tolist() == [10.0, 20.0]
    assert ptr.linear(A, None, x)[3].view(np.uint32).tolist() == [0, 0]  # +0: a chain started at +0 is never -0
    z = ptr.l2norm(np.array([[3.0, 4.0], [0.0, 0.0], [np.nan, 1.0]], dtype=np.float32))
    assert z[0].tolist() == [np.float32(3.0) * np.float32(0.2), np.float32(4.0) * np.float32(0.2)] and z[1].tolist() == [0.0, 0.0]
    assert np.isnan(z[2, 0]) and z[2, 1] == 1.0


def test_pretransform_apply_kernel_compiles_without_scratch():
    """from the compiler's own remarks (gfx950; no GPU needed): the eight instances of pretransform_apply_kernel -- 1 / 2 / 4 / 8 output tiles x
    aligned / unaligned rows -- use no scratch and spill no register; the widest keeps its 128 accumulator registers at one wave per SIMD"""
    import shutil
    import subprocess
    import tempfile

    import pytest

    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    csrc = os.path.join(ROOT, "duckdb-faiss-ext_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-I" + os.path.join(ROOT, "include"),
                            "-Rpass-analysis=kernel-resource-usage", "-c", "pretransform.hip", "-o", os.path.join(tmp, "pretransform.o")],
                           cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-4000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    inst = {n: u for n, u in kernels.items() if "pretransform_apply_kernel" in n}
    assert len(inst) == 8, sorted(inst)
    for name, u in kernels.items():
        if "pretransform" in name or "pca_" in name:
            assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0, (name, u)
    for name, u in inst.items():
        assert u["Occupancy"] >= (1 if "ILi8E" in name else 2), (name, u)
