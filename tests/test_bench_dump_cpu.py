"""bench.py --dump-outputs: what it writes for the last timed step -- float32 distances, float64 labels, at most DUMP_LIMIT_BYTES in
all, beyond that a fixed sample of query rows (the same for the same arguments, so two builds compare row for row).  Host only."""
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def bench():
    mp = pytest.MonkeyPatch()
    # (bench.py sets OMP_WAIT_POLICY's default when imported: not for the rest of the suite's OpenMP oracle)
    mp.setenv("OMP_WAIT_POLICY", os.environ.get("OMP_WAIT_POLICY", "passive"))
    import bench as b

    yield b
    mp.undo()


def _results(nq, k, seed):
    rs = np.random.RandomState(seed)
    D = np.sort(rs.rand(nq, k).astype(np.float32), axis=1)
    I = rs.randint(0, 10_000_000, size=(nq, k)).astype(np.int64)
    I[-1, -1] = -1  # (a missing result: FAISS's label -1)
    return D, I


def test_small_output_is_written_whole(bench, tmp_path):
    D, I = _results(37, 10, 0)
    bench.dump_outputs(str(tmp_path / "out"), D, I)
    Dd, Id = np.load(tmp_path / "out" / "distances.npy"), np.load(tmp_path / "out" / "labels.npy")
    assert Dd.dtype == np.float32 and Id.dtype == np.float64
    assert np.array_equal(Dd.view(np.uint32), D.view(np.uint32))
    assert np.array_equal(Id.astype(np.int64), I) and Id[-1, -1] == -1
    assert sorted(os.listdir(tmp_path / "out")) == ["distances.npy", "labels.npy"]


def test_large_output_is_a_fixed_sample_within_the_limit(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    D, I = _results(4000, 16, 1)  # 4000 x 16 x (4 + 8) bytes = 750 KB > 64 KB
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), D, I)
    files = ("distances.npy", "labels.npy", "query_rows.npy")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 10
    rows = np.load(tmp_path / "a" / "query_rows.npy")
    assert rows.dtype == np.float64 and len(rows) > 0 and np.all(np.diff(rows) > 0)
    r = rows.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "distances.npy"), D[r])
    assert np.array_equal(np.load(tmp_path / "a" / "labels.npy").astype(np.int64), I[r])
    for f in files:  # the same arguments give the same sample
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
