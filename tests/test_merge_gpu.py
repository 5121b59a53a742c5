"""merge_from and check_compatible_for_merge on the device (include/mi355_faiss.h "merge_from and copy_subset_to").

The yardstick is the same kind built in one go on the same parameters: it received A's rows, then B's rows in B's arrival order (an IVF kind:
add_with_ids(ids_B + add_id)).  After A.merge_from(B, add_id) A and the yardstick must agree in ntotal, in search (labels and distances bit
for bit, once with k beyond ntotal so that the padding is compared), in range_search where the kind has it, in the reconstruct family, in
the list getters and in every byte write_index produces.  One case per kind is also held against the CPU models (the oracle, pq_reference,
sq_reference, ivfpq_reference), so that both sides cannot be wrong together.

Shapes: for Flat every pair of interleave phases and both sides of a 32-row boundary (the pair-interleaved layout of d <= 128 depends on
bit 4 of the row number), two interleaved widths and a plain one; code pitches 16 and 32; inverted lists that are empty on one side only,
all of B in one list, duplicated explicit ids, a row in no list."""
import numpy as np
import pytest

from merge_helpers import (COARSE_KERNEL, IP, L2, PAIRS, assert_emptied, assert_indistinguishable, assert_matches_model, circle, fill, is_ivf, make,
                           orc, params_of, queries_of, rows_of, u32)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss as m

    assert m.device_count() >= 1
    return m


# ---------------------------------------------------------------------------------------------------------------- Flat
FLAT_CASES = [(L2, d, na, nb) for d in (8, 128, 132) for na, nb in PAIRS] + [(IP, 8, na, nb) for na, nb in PAIRS]


@pytest.mark.parametrize("metric,d,na,nb", FLAT_CASES)
def test_flat(mf, tmp_path, metric, d, na, nb):
    xa, xb = rows_of(d, na, 1), rows_of(d, nb, 2)
    a, b, y = (mf.index_factory(d, "Flat", metric) for _ in range(3))
    fill(a, xa), fill(b, xb), fill(y, xa), fill(y, xb)
    a.check_compatible_for_merge(b)
    a.merge_from(b)
    what = f"Flat d {d} metric {metric} {na}+{nb}"
    assert_indistinguishable(mf, a, y, "Flat", d, tmp_path, what)
    assert_emptied(mf, b, "Flat", d, what)
    if (na, nb) == (17, 16):
        assert_matches_model(a, "Flat", d, metric, np.concatenate([xa, xb]), None, None, what)


def test_flat_rows_still_staged_on_both_sides(mf, tmp_path):
    """small chunked adds stay in the pinned staging slot until something reads the rows: the merge is that reader, on both sides"""
    d = 8
    xa, xb = rows_of(d, 37, 3), rows_of(d, 29, 4)
    a, b, y = (mf.index_factory(d, "Flat", L2) for _ in range(3))
    for i in range(0, 37, 5):
        a.add(xa[i : i + 5])
    for i in range(0, 29, 3):
        b.add(xb[i : i + 3])
    fill(y, xa), fill(y, xb)
    a.merge_from(b)
    assert_indistinguishable(mf, a, y, "Flat", d, tmp_path, "staged")
    assert_matches_model(a, "Flat", d, L2, np.concatenate([xa, xb]), None, None, "staged")


def test_flat_searched_through_the_coarse_filter_before_the_merge(mf):
    """the destination's derived coarse store covers its old rows only: it must be extended, not trusted (4096 rows: the smallest index the
    forced coarse filter takes)"""
    d, na, nb, k = 64, 4096, 1017, 10
    rng = np.random.default_rng(5)
    xa, xb = rng.random((na, d), dtype=np.float32), rng.random((nb, d), dtype=np.float32)
    xq = np.concatenate([rng.random((24, d), dtype=np.float32), xb[:8] + np.float32(1e-3)])  # (some answers lie among the merged rows)
    a, b, y = (mf.index_factory(d, "Flat", L2) for _ in range(3))
    for ix in (a, y):
        ix.set_option("prefilter", 2)
    a.add(xa), b.add(xb), y.add(xa), y.add(xb)
    a.search(xq, k)
    assert a.last_kernel_info()["name"] == COARSE_KERNEL
    a.merge_from(b)
    D, I = a.search(xq, k)
    assert a.last_kernel_info()["name"] == COARSE_KERNEL
    Dy, Iy = y.search(xq, k)
    assert np.array_equal(I, Iy) and np.array_equal(u32(D), u32(Dy))
    Do, Io = orc.flat_search(L2, np.concatenate([xa, xb]), xq, k)
    assert np.array_equal(I, Io) and np.array_equal(u32(D), u32(Do))
    assert (I[24:, 0] >= na).all()


# ---------------------------------------------------------------------------------------------------------------- PQ4, SQ8
@pytest.mark.parametrize("desc", ["PQ4", "SQ8"])
@pytest.mark.parametrize("d", [8, 20])
@pytest.mark.parametrize("na,nb", [(0, 5), (5, 0), (16, 17), (31, 33)])
def test_codes(mf, tmp_path, desc, d, na, nb):
    xa, xb = rows_of(d, na, 1), rows_of(d, nb, 2)
    a, b, y = (make(mf, desc, d) for _ in range(3))
    fill(a, xa), fill(b, xb), fill(y, xa), fill(y, xb)
    a.merge_from(b)
    what = f"{desc} d {d} {na}+{nb}"
    assert_indistinguishable(mf, a, y, desc, d, tmp_path, what)
    assert_emptied(mf, b, desc, d, what)
    if (na, nb) == (16, 17):
        assert_matches_model(a, desc, d, L2, np.concatenate([xa, xb]), None, None, what)


# ---------------------------------------------------------------------------------------------------------------- IVF4 over Flat, PQ2, SQ8
def ivf_case(name):
    """(lists of A's rows, lists of B's rows, explicit ids?)"""
    rng = np.random.default_rng(len(name))
    counts = {"one_side_empty": ([5, 0, 7, 3], [0, 6, 2, 0]), "b_in_one_list": ([4, 4, 4, 4], [0, 0, 9, 0]), "duplicate_ids": ([6, 5, 4, 3], [3, 4, 5, 6])}[name]
    la, lb = (tuple(int(v) for v in rng.permutation(np.repeat(np.arange(4), c))) for c in counts)
    return la, lb, name == "duplicate_ids"


@pytest.mark.parametrize("desc", ["IVF4,Flat", "IVF4,PQ2", "IVF4,SQ8"])
@pytest.mark.parametrize("case", ["one_side_empty", "b_in_one_list", "duplicate_ids"])
@pytest.mark.parametrize("add_id", [0, 1000])
def test_ivf(mf, tmp_path, desc, case, add_id):
    d = 8
    la, lb, explicit = ivf_case(case)
    xa, xb = rows_of(d, len(la), 1, la), rows_of(d, len(lb), 2, lb)
    rng = np.random.default_rng(11)
    ia = rng.integers(0, 10, len(la)) if explicit else None
    ib = rng.integers(0, 10, len(lb)) if explicit else np.arange(len(lb))
    a, b, y = (make(mf, desc, d) for _ in range(3))
    fill(a, xa, ia), fill(b, xb, ib if explicit else None), fill(y, xa, ia), fill(y, xb, ib + add_id)
    a.check_compatible_for_merge(b)
    a.merge_from(b, add_id)
    what = f"{desc} {case} add_id {add_id}"
    stored = np.concatenate([ia if explicit else np.arange(len(la)), ib + add_id])
    assert_indistinguishable(mf, a, y, desc, d, tmp_path, what, keys=stored, nprobes=(1, 4))
    assert_emptied(mf, b, desc, d, what)
    if case == "one_side_empty":
        assert_matches_model(a, desc, d, L2, np.concatenate([xa, xb]), stored, None, what)
        assert_matches_model(a, desc, d, L2, np.concatenate([xa, xb]), stored, None, what, nprobe=1)


@pytest.mark.parametrize("desc", ["IVF4,Flat", "IVF4,PQ2", "IVF4,SQ8", "IVF4_HNSW8,Flat"])
def test_ivf_row_in_no_list_travels_as_it_is(mf, tmp_path, desc):
    """a row of NaN has no nearest centroid: its directory label is -1 on both sides of the merge"""
    d = 8
    la, lb, _ = ivf_case("one_side_empty")
    xa, xb = rows_of(d, len(la), 1, la), rows_of(d, len(lb), 2, lb).copy()
    if "HNSW" not in desc:
        xb[3] = np.nan
    a, b, y = (make(mf, desc, d) for _ in range(3))
    fill(a, xa), fill(b, xb), fill(y, xa), fill(y, xb, np.arange(len(lb)) + 50)
    a.merge_from(b, 50)
    assert a.ntotal == len(la) + len(lb)
    keep = np.array([i for i in range(len(lb)) if i != 3 or "HNSW" in desc])
    assert_indistinguishable(mf, a, y, desc, d, tmp_path, desc, keys=np.concatenate([np.arange(len(la)), keep + 50]), nprobes=(4,))


def test_ivf_ids_ascending_stays_truthful(mf):
    d = 8
    la, lb, _ = ivf_case("one_side_empty")
    xa, xb = rows_of(d, len(la), 1, la), rows_of(d, len(lb), 2, lb)
    for add_id, want in ((len(la), 1), (len(la) - 1, 0), (0, 0)):
        a, b = make(mf, "IVF4,Flat", d), make(mf, "IVF4,Flat", d)
        a.add(xa), b.add(xb)
        a.merge_from(b, add_id)
        assert a.get_stat("ivf_ids_ascending") == want, add_id
        assert b.get_stat("ivf_ids_ascending") == 1
    a, b = make(mf, "IVF4,Flat", d), make(mf, "IVF4,Flat", d)
    a.add(xa), b.add_with_ids(xb, np.arange(len(lb))[::-1] + 100)  # (B's own ids descend)
    a.merge_from(b)
    assert a.get_stat("ivf_ids_ascending") == 0


# ---------------------------------------------------------------------------------------------------------------- IDMap, IDMap2
@pytest.mark.parametrize("wrap", ["IDMap", "IDMap2"])
@pytest.mark.parametrize("base", ["Flat", "IVF4,Flat", "PQ4", "IVF4,SQ8"])
@pytest.mark.parametrize("add_id", [0, 7])
def test_idmap(mf, tmp_path, wrap, base, add_id):
    d, desc = 8, f"{wrap},{base}"
    la, lb, _ = ivf_case("one_side_empty")
    ivf = base.startswith("IVF")
    xa, xb = rows_of(d, len(la), 1, la if ivf else None), rows_of(d, len(lb), 2, lb if ivf else None)
    ea, eb = 100 + 3 * np.arange(len(la)), (5000 - 7 * np.arange(len(lb))) % 4990  # external ids, not ascending
    eb[2] = ea[4] - add_id  # one external id on both sides after the shift: legal
    a, b, y = (make(mf, desc, d) for _ in range(3))
    fill(a, xa, ea), fill(b, xb, eb), fill(y, xa, ea), fill(y, xb, eb + add_id)
    a.check_compatible_for_merge(b)
    a.merge_from(b, add_id)
    what = f"{desc} add_id {add_id}"
    ext = np.concatenate([ea, eb + add_id])
    assert a.index.ntotal == len(ext)
    assert_indistinguishable(mf, a, y, desc, d, tmp_path, what, keys=ext, nprobes=(1, 4))
    assert_emptied(mf, b, desc, d, what)
    if wrap == "IDMap":
        assert_matches_model(a, desc, d, L2, np.concatenate([xa, xb]), None, ext, what)


# ---------------------------------------------------------------------------------------------------------------- afterwards
@pytest.mark.parametrize("desc", ["Flat", "PQ4", "SQ8", "IVF4,Flat", "IVF4,PQ2", "IVF4,SQ8", "IDMap,Flat", "IDMap,IVF4,Flat"])
def test_afterwards_both_indexes_live_on(mf, tmp_path, desc):
    """B takes new rows and answers like a fresh index; A merges a third index; remove_ids works on the merged A"""
    d = 8
    ivf, idm = is_ivf(desc), desc.startswith("IDMap")
    lists = [tuple(int(v) for v in np.random.default_rng(s).integers(0, 4, n)) for s, n in ((1, 21), (2, 18), (3, 9), (4, 12))]
    xs = [rows_of(d, len(l), 10 + i, l if ivf else None) for i, l in enumerate(lists)]
    first = np.cumsum([0] + [len(x) for x in xs])
    ids = [200 + first[i] + np.arange(len(x)) if idm else None for i, x in enumerate(xs)]
    a, b, c, y, fresh = (make(mf, desc, d) for _ in range(5))
    fill(a, xs[0], ids[0]), fill(b, xs[1], ids[1]), fill(c, xs[2], ids[2])
    shift = (lambda i: int(first[i])) if ivf and not idm else (lambda i: 0)  # (a bare IVF kind numbers every part from 0)
    a.merge_from(b, shift(1))
    fill(b, xs[3], ids[3]), fill(fresh, xs[3], ids[3])
    keys3 = ids[3] if idm else (np.arange(len(xs[3])) if ivf else None)
    assert_indistinguishable(mf, b, fresh, desc, d, tmp_path, f"{desc}: B refilled", keys=keys3, nprobes=(4,))
    a.merge_from(c, shift(2))
    assert c.ntotal == 0
    for i in range(3):
        fill(y, xs[i], ids[i] if idm else (first[i] + np.arange(len(xs[i])) if ivf else None))
    labels = np.arange(first[3]) + (200 if idm else 0)
    assert_indistinguishable(mf, a, y, desc, d, tmp_path, f"{desc}: three parts", keys=labels if (ivf or idm) else None, nprobes=(4,))
    gone = ("batch", labels[::3].astype(np.int64))
    assert a.remove_ids(gone) == y.remove_ids(gone) == len(labels[::3])
    left = np.setdiff1d(labels, labels[::3])
    assert_indistinguishable(mf, a, y, desc, d, tmp_path, f"{desc}: after remove_ids", keys=left if (ivf or idm) else None, nprobes=(4,))


# ---------------------------------------------------------------------------------------------------------------- refusals
def answers(ix, d, ivf):
    if not ix.is_trained:
        return (ix.ntotal,)
    D, I = ix.search(queries_of(d, 5, ivf), 6, nprobe=4)
    return ix.ntotal, u32(D).tobytes(), I.tobytes()


def one_bit(a):
    b = np.array(a, dtype=np.float32, copy=True)
    b.reshape(-1).view(np.uint32)[-1] ^= 1
    return b


def refusal_cases():
    P = params_of
    # (A: desc, d, metric, parameters or None) (B: ...) text of the refusal
    yield ("Flat", 8, L2, None), ("Flat", 12, L2, None), "d differs"
    yield ("Flat", 8, L2, None), ("Flat", 8, IP, None), "metric differs"
    yield ("Flat", 8, L2, None), ("SQ8", 8, L2, None), "kinds differ"
    yield ("IVF4,Flat", 8, L2, None), ("IVF4,SQ8", 8, L2, None), "kinds differ"
    yield ("IVF4,Flat", 8, L2, None), ("IVF3,Flat", 8, L2, {"cent": circle(3, 8)}), "nlist differs"
    yield ("IVF4,Flat", 8, L2, None), ("IVF4_HNSW8,Flat", 8, L2, None), "quantizers differ"
    yield ("PQ4", 8, L2, None), ("PQ2", 8, L2, None), "M differs"
    yield ("IVF4,PQ2", 8, L2, None), ("IVF4,PQ4", 8, L2, None), "code size differs"
    yield ("IVF4,Flat", 8, L2, None), ("IVF4,Flat", 8, L2, {"cent": one_bit(circle(4, 8))}), "coarse centroids differ"
    yield ("IVF4,SQ8", 8, L2, None), ("IVF4,SQ8", 8, L2, dict(P("IVF4,SQ8", 8), cent=one_bit(circle(4, 8)))), "coarse centroids differ"
    yield ("PQ4", 8, L2, None), ("PQ4", 8, L2, {"cb": one_bit(P("PQ4", 8)["cb"])}), "codebooks differ"
    yield ("IVF4,PQ2", 8, L2, None), ("IVF4,PQ2", 8, L2, dict(P("IVF4,PQ2", 8), cb=one_bit(P("IVF4,PQ2", 8)["cb"]))), "codebooks differ"
    yield ("SQ8", 8, L2, None), ("SQ8", 8, L2, {"sq": (P("SQ8", 8)["sq"][0], one_bit(P("SQ8", 8)["sq"][1]))}), "ranges differ"
    yield ("IDMap,Flat", 8, L2, None), ("IDMap2,Flat", 8, L2, None), "IDMap against IDMap2"
    yield ("IDMap,Flat", 8, L2, None), ("Flat", 8, L2, None), "kinds differ"
    yield ("IDMap,PQ4", 8, L2, None), ("IDMap,PQ4", 8, L2, {"cb": one_bit(P("PQ4", 8)["cb"])}), "codebooks differ"


@pytest.mark.parametrize("A,B,text", list(refusal_cases()), ids=lambda v: v if isinstance(v, str) else v[0] + "-" + str(v[1]))
def test_incompatible_indexes_are_refused_and_stay_untouched(mf, A, B, text):
    ixs = []
    for desc, d, metric, p in (A, B):
        ix = make(mf, desc, d, metric, p)
        ivf = is_ivf(desc)
        x = rows_of(d, 19, 5, tuple(i % 4 for i in range(19)) if ivf else None)
        fill(ix, x, 300 + np.arange(19) if desc.startswith("IDMap") else None)
        ixs.append((ix, d, ivf))
    before = [answers(*t) for t in ixs]
    for call in (lambda: ixs[0][0].check_compatible_for_merge(ixs[1][0]), lambda: ixs[0][0].merge_from(ixs[1][0])):
        with pytest.raises(mf.FaissException, match=text):
            call()
    assert [answers(*t) for t in ixs] == before


def test_untrained_side_self_and_add_id_are_refused(mf):
    d = 8
    x = rows_of(d, 19, 5, tuple(i % 4 for i in range(19)))
    a = make(mf, "IVF4,PQ2", d)
    a.add(x)
    for p in ({}, {"cent": circle(4, d)}):  # nothing trained; centroids without codebooks
        u = mf.index_factory(d, "IVF4,PQ2", L2)
        if p:
            u.ivf_set_centroids(p["cent"])
        assert not u.is_trained
        before = answers(a, d, True)
        for dst, src, text in ((a, u, "the other index is not trained"), (u, a, "this index is not trained")):
            for call in (lambda: dst.merge_from(src), lambda: dst.check_compatible_for_merge(src)):
                with pytest.raises(mf.FaissException, match=text):
                    call()
        assert answers(a, d, True) == before and u.ntotal == 0 and not u.is_trained
    up = mf.index_factory(d, "PQ4", L2)
    with pytest.raises(mf.FaissException, match="the other index is not trained"):
        make(mf, "PQ4", d).merge_from(up)
    before = answers(a, d, True)
    for call in (lambda: a.merge_from(a), lambda: a.check_compatible_for_merge(a)):
        with pytest.raises(mf.FaissException, match="other == this"):
            call()
    assert answers(a, d, True) == before
    for desc in ("Flat", "PQ4", "SQ8"):
        p, q = make(mf, desc, d), make(mf, desc, d)
        p.add(rows_of(d, 19, 5)), q.add(rows_of(d, 7, 6))
        before = answers(p, d, False), answers(q, d, False)
        with pytest.raises(mf.FaissException, match="cannot set ids in FlatCodes index"):
            p.merge_from(q, 3)
        assert (answers(p, d, False), answers(q, d, False)) == before


@pytest.mark.parametrize("desc", ["HNSW8", "SQ8,RFlat", "PCA4,Flat", "sharded"])
def test_kinds_without_merge_refuse_with_the_base_class_texts(mf, desc):
    d = 8
    x = rows_of(d, 300, 7)
    ixs = []
    for _ in range(2):
        ix = mf.index_factory(d, "Flat" if desc == "sharded" else desc, L2)
        if not ix.is_trained:
            ix.train(x)
        ix.add(x[:40])
        if desc == "sharded":
            ix.shard_to_gpus([0, 0])
        ixs.append(ix)
    before = [answers(ix, d, False) for ix in ixs]
    with pytest.raises(mf.FaissException, match=r"merge_from\(\) not implemented"):
        ixs[0].merge_from(ixs[1])
    with pytest.raises(mf.FaissException, match=r"check_compatible_for_merge\(\) not implemented"):
        ixs[0].check_compatible_for_merge(ixs[1])
    plain = mf.index_factory(d, "Flat", L2)
    plain.add(x[:5])
    with pytest.raises(mf.FaissException):  # (nor does a served kind take one of them)
        plain.merge_from(ixs[1])
    assert plain.ntotal == 5 and [answers(ix, d, False) for ix in ixs] == before


# ---------------------------------------------------------------------------------------------------------------- adaptor and driver
@pytest.mark.parametrize("desc", ["IDMap,Flat", "IDMap,IVF4,Flat"])
def test_boundary_driver_merge(desc):
    """the compat faiss::Index::merge_from through host/boundary_driver: two threads each fill a private index, the parts are merged, and
    the result answers bit for bit like one index filled under the lock"""
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "duckdb-faiss-ext_amd", "host", "boundary_driver")
    assert os.path.exists(exe), "host/boundary_driver is built by build()"
    r = subprocess.run([exe, "merge", "3000", "16", "9", desc], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and "MERGE OK" in r.stdout, r.stdout[-3000:]
