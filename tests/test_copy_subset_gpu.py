"""copy_subset_to on the device (include/mi355_faiss.h "merge_from and copy_subset_to"): the three bare IVF kinds, nlist 4,
d = 8, 60 rows under explicit ids with negatives and duplicates.  The yardstick is the destination built by add_with_ids of the rows a
numpy predicate selects, in the source's order: lists, search bits and file bytes must agree, and the source's file must not change.  The
element-range type is restated from FAISS from memory (UNVERIFIED in the header); what is tested for it does not depend on memory: the
formula as the header states it, and that thirds of [0, ntotal) put every listed row in exactly one part -- which holds here because no
third meets a list with an inverted range (lists of 26, 5, 17 and 12 rows: the cuts are 8 | 17, 2 | 3, 6 | 12, 4 | 8); the header and
tests/test_directory_merge_cpu.py have the general rule."""
import numpy as np
import pytest

from merge_helpers import assert_indistinguishable, circle, file_bytes, fill, lists_of, make, queries_of, rows_of, u32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss as m

    assert m.device_count() >= 1
    return m


KINDS = ["IVF4,Flat", "IVF4,PQ2", "IVF4,SQ8"]
D, N = 8, 60
ID_RANGE, ID_MOD, ELEMENT_RANGE = 0, 1, 2


def source_rows(unique=False):
    rng = np.random.default_rng(60)
    lists = tuple(int(v) for v in rng.choice(4, N, p=[0.4, 0.1, 0.3, 0.2]))
    ids = np.arange(N, dtype=np.int64) * 7 - 100 if unique else rng.integers(-20, 25, N).astype(np.int64)  # negatives (and duplicates)
    return rows_of(D, N, 60 + unique, lists), ids


def row_lists(x):
    """the list of every source row: the nearest centroid (the centroids are 100 apart, the rows within 1 of one: no doubt about it)"""
    return np.argmin(((x[:, None, :].astype(np.float64) - circle(4, D)[None]) ** 2).sum(-1), axis=1)


def element_range_mask(of, a1, a2, ntotal):
    """the header's formula, written out"""
    keep = np.zeros(len(of), dtype=bool)
    accu_n = accu_a1 = accu_a2 = 0
    for l in range(4):
        rows = np.flatnonzero(of == l)
        next_n = accu_n + len(rows)
        i1, i2 = next_n * a1 // ntotal - accu_a1, next_n * a2 // ntotal - accu_a2
        keep[rows[i1:i2]] = True
        accu_n, accu_a1, accu_a2 = next_n, accu_a1 + i1, accu_a2 + i2
    return keep


def c_mod(ids, a1):
    return np.fmod(ids, a1)  # (C's %: the sign of the dividend)


@pytest.mark.parametrize("desc", KINDS)
@pytest.mark.parametrize("subset", [(ID_RANGE, -5, 12), (ID_RANGE, 100, 200), (ID_MOD, 3, 1), (ID_MOD, 3, -2), (ELEMENT_RANGE, 0, 20), (ELEMENT_RANGE, 20, 47)])
@pytest.mark.parametrize("filled", [False, True])
def test_subset_equals_add_with_ids_of_the_selected_rows(mf, tmp_path, desc, subset, filled):
    t, a1, a2 = subset
    x, ids = source_rows()
    src, dst, y = (make(mf, desc, D) for _ in range(3))
    src.add_with_ids(x, ids)
    if filled:
        x0 = rows_of(D, 9, 3, (0, 1, 2, 3, 0, 1, 2, 3, 0))
        fill(dst, x0, 900 + np.arange(9)), fill(y, x0, 900 + np.arange(9))
    before = file_bytes(mf, src, tmp_path, "src0.index")
    if t == ID_RANGE:
        keep = (ids >= a1) & (ids < a2)
    elif t == ID_MOD:
        keep = c_mod(ids, a1) == a2
    else:
        keep = element_range_mask(row_lists(x), a1, a2, N)
    src.copy_subset_to(dst, t, a1, a2)
    fill(y, x[keep], ids[keep])
    assert keep.any() == (subset != (ID_RANGE, 100, 200))
    keys = np.concatenate([ids[keep], 900 + np.arange(9) if filled else []]).astype(np.int64)
    if dst.ntotal:
        assert_indistinguishable(mf, dst, y, desc, D, tmp_path, f"{desc} {subset} filled {filled}", keys=keys, nprobes=(1, 4))
    else:
        assert y.ntotal == 0
    assert file_bytes(mf, src, tmp_path, "src1.index") == before, "the source changed"


def entries(ix, desc):
    """the (id, code) multiset of every list"""
    return [sorted((int(i), bytes(np.ascontiguousarray(c))) for i, c in zip(*l)) for l in lists_of(ix, desc)]


@pytest.mark.parametrize("desc", ["IVF4,PQ2", "IVF4,SQ8"])
@pytest.mark.parametrize("how", ["mod", "elements"])
def test_partition_and_merge_back(mf, tmp_path, desc, how):
    """type 1 with a1 = 3 and a2 = 0, 1, 2 -- over ids that are not negative, where C's % has three values --, and type 2 over thirds of
    [0, ntotal): every listed row lands in exactly one part, and the parts merged back hold the source's lists"""
    x, ids = source_rows(unique=True)
    ids = ids + 100  # 0, 7, 14, ...
    src = make(mf, desc, D)
    src.add_with_ids(x, ids)
    calls = [(ID_MOD, 3, r) for r in range(3)] if how == "mod" else [(ELEMENT_RANGE, N * i // 3, N * (i + 1) // 3) for i in range(3)]
    parts = []
    for t, a1, a2 in calls:
        p = make(mf, desc, D)
        src.copy_subset_to(p, t, a1, a2)
        parts.append(p)
    assert sum(p.ntotal for p in parts) == N and all(p.ntotal > 0 for p in parts)
    seen = np.concatenate([np.concatenate([i for i, _ in lists_of(p, desc)]) for p in parts])
    assert np.array_equal(np.sort(seen), np.sort(ids)), "a row is in no part, or in two"
    back = make(mf, desc, D)
    for p in parts:
        back.merge_from(p)
    assert back.ntotal == N and entries(back, desc) == entries(src, desc)


def test_partition_and_merge_back_ivfflat_searches_alike(mf, tmp_path):
    """IVF4,Flat on data without ties: the parts merged back answer like the source (list order may differ, values and labels may not)"""
    desc = "IVF4,Flat"
    rng = np.random.default_rng(8)
    lists = rng.integers(0, 4, N)
    x = (circle(4, D)[lists] + rng.uniform(-0.5, 0.5, (N, D))).astype(np.float32)
    ids = np.arange(N, dtype=np.int64) * 7
    for calls in ([(ID_MOD, 3, r) for r in range(3)], [(ELEMENT_RANGE, N * i // 3, N * (i + 1) // 3) for i in range(3)]):
        src, back = make(mf, desc, D), make(mf, desc, D)
        src.add_with_ids(x, ids)
        total = 0
        for t, a1, a2 in calls:
            p = make(mf, desc, D)
            src.copy_subset_to(p, t, a1, a2)
            total += p.ntotal
            back.merge_from(p)
        assert total == N == back.ntotal
        xq = queries_of(D, 25, True)
        for nprobe in (1, 4):
            Da, Ia = src.search(xq, 5, nprobe=nprobe)
            Db, Ib = back.search(xq, 5, nprobe=nprobe)
            assert np.array_equal(Ia, Ib) and np.array_equal(u32(Da), u32(Db))
        assert np.array_equal(u32(src.reconstruct_batch(ids)), u32(back.reconstruct_batch(ids)))


def test_refusals(mf):
    x, ids = source_rows()
    src, dst = make(mf, "IVF4,Flat", D), make(mf, "IVF4,Flat", D)
    src.add_with_ids(x, ids)
    for t in (3, 4, -1, 17):
        with pytest.raises(mf.FaissException, match="subset type not implemented"):
            src.copy_subset_to(dst, t, 0, 10)
    for a1 in (0, -3):
        with pytest.raises(mf.FaissException, match="a1 > 0"):
            src.copy_subset_to(dst, ID_MOD, a1, 0)
    with pytest.raises(mf.FaissException, match="nlist differs"):
        src.copy_subset_to(make(mf, "IVF3,Flat", D, p={"cent": circle(3, D)}), ID_RANGE, -100, 100)
    with pytest.raises(mf.FaissException, match="kinds differ"):
        src.copy_subset_to(make(mf, "IVF4,SQ8", D), ID_RANGE, -100, 100)
    moved = circle(4, D)
    moved[0, 0] += 1
    with pytest.raises(mf.FaissException, match="coarse centroids differ"):
        src.copy_subset_to(make(mf, "IVF4,Flat", D, p={"cent": moved}), ID_RANGE, -100, 100)
    with pytest.raises(mf.FaissException, match="other == this"):
        src.copy_subset_to(src, ID_RANGE, -100, 100)
    assert dst.ntotal == 0 and src.ntotal == N
    for desc in ("Flat", "SQ8", "IDMap,IVF4,Flat"):  # (the bare IVF kinds only)
        a, b = make(mf, desc, D), make(mf, desc, D)
        with pytest.raises(mf.FaissException, match="bare IVF kinds only"):
            a.copy_subset_to(b, ID_RANGE, 0, 10)
