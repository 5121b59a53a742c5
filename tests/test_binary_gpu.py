"""Binary indexes on the device (include/mi355_faiss.h "binary indexes") against the CPU model of tests/binary_reference.py.
Everything is compared bit for bit: distances are integers.  The shapes are the smallest that reach each edge: word tails (d = 8, 24, 72,
264), one row, a tile edge (63 / 64 / 65 rows), several tiles and generations (4097), k beyond the rows, ties that only the pair bound keeps
apart, stream overflow, selectors that starve the list, staged adds."""
import os
import subprocess

import numpy as np
import pytest

import binary_reference as br

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "duckdb-faiss-ext_amd", "host", "boundary_driver")
PAD = 2147483647


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss as m

    assert m.device_count() >= 1
    return m


def codes(seed, n, d):
    return np.random.default_rng(seed).integers(0, 256, (n, d // 8), dtype=np.uint8)


def build(mf, d, xb, ids=None, desc=None):
    ix = mf.index_binary_factory(d, desc or ("BFlat" if ids is None else "IDMap,BFlat"))
    if ids is None:
        ix.add(xb)
    else:
        ix.add_with_ids(xb, ids)
    return ix


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].dtype == np.int32 and got[1].dtype == np.int64


def bitmap_of(ids):
    ids = np.asarray(ids, dtype=np.int64)
    bits = np.zeros(int(ids.max()) // 8 + 1, dtype=np.uint8)
    np.bitwise_or.at(bits, ids >> 3, (1 << (ids & 7)).astype(np.uint8))
    return bits


# ---- word tails and sizes
@pytest.mark.parametrize("d", [8, 24, 64, 72, 256, 264, 1024, 2048])
def test_word_tails_and_sizes(mf, d):
    xq_all = codes(100 + d, 129, d)
    for n, nq, k in [(1, 1, 1), (1, 17, 10), (63, 17, 100), (64, 1, 10), (65, 129, 10), (4097, 17, 100), (4097, 129, 1), (4097, 1, 10)]:
        if d >= 1024 and n == 4097 and nq == 129:
            nq = 33  # (the model's distance matrix, not the device, sets the pace at 2048 bits)
        xb = codes(d + n, n, d)
        xb[n // 2] = xq_all[0]  # a planted exact match
        ix = build(mf, d, xb)
        assert ix.ntotal == n and ix.d == d and ix.code_size == d // 8 and ix.kind == mf.BINARY_KIND_FLAT
        assert same(ix.search(xq_all[:nq], k), br.search(xb, xq_all[:nq], k)), (d, n, nq, k)


def test_d8_has_nine_distances_among_4097_rows(mf):
    xb, xq = codes(1, 4097, 8), codes(2, 129, 8)
    ix = build(mf, 8, xb)
    dist = br.ham(xq, xb)
    for k in (1, 10, 100):
        got = ix.search(xq, k)
        assert same(got, br.search(xb, xq, k, dist=dist)), k
    assert len(np.unique(got[0])) <= 9 and ix.get_stat("binary_scan_launches") >= 2


# ---- ties
@pytest.mark.parametrize("d", [8, 256])
def test_ties_every_row_identical(mf, d):
    row = codes(5, 1, d)
    xb = np.repeat(row, 5000, axis=0)
    ix = build(mf, d, xb)
    ix.set_option("binary_first_rows", 64)
    xq = codes(6, 7, d)
    D, I = ix.search(xq, 100)
    assert np.array_equal(I, np.tile(np.arange(100), (7, 1))) and np.array_equal(D, np.repeat(br.ham(xq, row), 100, axis=1))
    # the pair bound admits nothing after row k - 1: the stream holds the first generation's rows (128: at least k, whole tiles) and no more
    assert ix.get_stat("binary_candidates") == 7 * 128 and ix.get_stat("binary_scan_launches") >= 3


def test_ties_four_distinct_codes(mf):
    base = codes(7, 4, 64)
    xb = base[np.random.default_rng(8).integers(0, 4, 5000)]
    xq = np.concatenate([base, codes(9, 13, 64)])
    ix = build(mf, 64, xb)
    assert same(ix.search(xq, 100), br.search(xb, xq, 100))


@pytest.mark.parametrize("d", [8, 72, 2048])
def test_ties_all_ones_query_against_zero_rows(mf, d):
    xb = np.zeros((300, d // 8), dtype=np.uint8)
    xq = np.full((3, d // 8), 0xFF, dtype=np.uint8)
    D, I = build(mf, d, xb).search(xq, 10)
    assert np.all(D == d) and np.array_equal(I, np.tile(np.arange(10), (3, 1)))


# ---- generations and overflow
@pytest.fixture(scope="module")
def big():
    xb, xq = codes(11, 70000, 256), codes(12, 300, 256)
    xb[60000:60300] = xq  # late exact matches: every query's list changes in the last generation
    return xb, xq, br.search(xb, xq, 10)


def test_generations_and_stream_overflow(mf, big):
    xb, xq, want = big
    ix = build(mf, 256, xb)
    ix.set_option("binary_first_rows", 256)
    assert same(ix.search(xq, 10), want)
    launches, cand = ix.get_stat("binary_scan_launches"), ix.get_stat("binary_candidates")
    assert launches >= 5 and ix.get_stat("binary_rescans") == 0  # 256, 1024, 4096, 16384, 65536, 70000
    assert 300 * 256 <= cand < 300 * 1000  # the first rows, then about 3 k records per query and generation (a generation is 3 x the rows before it)
    ix.set_option("binary_stream_cap", 64)
    assert same(ix.search(xq, 10), want)
    assert ix.get_stat("binary_rescans") > 0 and ix.get_stat("binary_candidates") == cand
    ix.set_option("binary_stream_cap", 0)
    ix.set_option("binary_first_rows", 5000)  # other generations, the same result
    assert same(ix.search(xq, 10), want) and ix.get_stat("binary_scan_launches") < launches


def test_k_2048_and_k_limits(mf):
    xb, xq = codes(13, 20000, 64), codes(14, 5, 64)
    ix = build(mf, 64, xb)
    assert same(ix.search(xq, 2048), br.search(xb, xq, 2048))
    with pytest.raises(mf.FaissException, match="beyond the largest k"):
        ix.search(xq, 2049)
    with pytest.raises(mf.FaissException, match="'k > 0' failed"):
        ix.search(xq, 0)
    D, I = ix.search(xq[:0], 3)  # n == 0 is a no-op
    assert D.shape == (0, 3)


def test_empty_index_pads_everything(mf):
    for desc in ("BFlat", "IDMap,BFlat"):
        D, I = mf.index_binary_factory(64, desc).search(codes(1, 3, 64), 4)
        assert np.all(D == PAD) and np.all(I == -1)


# ---- selectors
@pytest.fixture(scope="module")
def seldata():
    xb, xq = codes(21, 3000, 72), codes(22, 33, 72)
    ids = np.random.default_rng(23).permutation(50000)[:3000].astype(np.int64) * 3 - 1000  # scattered, some negative
    return xb, xq, ids, br.ham(xq, xb)


@pytest.mark.parametrize("idmap", [False, True])
@pytest.mark.parametrize("kind", ["bitmap", "batch"])
def test_selectors(mf, seldata, idmap, kind):
    xb, xq, ids, dist = seldata
    lab = ids if idmap else np.arange(3000, dtype=np.int64)
    ix = build(mf, 72, xb, ids if idmap else None)
    rng = np.random.default_rng(24)
    pos = lab[lab >= 0]
    for name, chosen in [("third", rng.choice(pos, pos.size // 3, replace=False)), ("fewer than k", pos[:4]), ("one", pos[5:6])]:
        if kind == "bitmap":
            sel = ("bitmap", bitmap_of(chosen))
        else:
            sel = ("batch", np.concatenate([chosen, chosen[:2], [10**12]]))  # duplicates and a stranger
        got = ix.search(xq, 10, sel=sel)
        assert same(got, br.search(xb, xq, 10, sel=sel, id_map=lab if idmap else None, dist=dist)), name
        assert np.isin(got[1][got[1] >= 0], chosen).all()
    none = ("bitmap", np.zeros(4, np.uint8)) if kind == "bitmap" else ("batch", np.array([10**12, -8]))  # (no id is 3 p - 1000 = -8)
    D, I = ix.search(xq, 10, sel=none)
    assert np.all(D == PAD) and np.all(I == -1)
    if idmap:  # the wrapped index: labels and the selector's ids are row numbers
        sel = ("batch", np.arange(0, 3000, 7))
        assert ix.index.kind == mf.BINARY_KIND_FLAT and ix.kind == mf.BINARY_KIND_IDMAP
        assert same(ix.index.search(xq, 10, sel=sel), br.search(xb, xq, 10, sel=sel, dist=dist))


# ---- staging
def test_staged_adds_are_seen_by_every_reader(mf):
    rng = np.random.default_rng(31)
    xq = codes(32, 9, 264)
    ix = mf.index_binary_factory(264, "IDMap2,BFlat")
    rows, ids = [], []
    for step in range(37):
        n = int(rng.integers(1, 301))
        x = rng.integers(0, 256, (n, 33), dtype=np.uint8)
        i = rng.integers(0, 1 << 40, n)
        ix.add_with_ids(x, i)
        rows.append(x), ids.append(i)
        if step % 6 == 5 or step == 36:
            xb, lab = np.concatenate(rows), np.concatenate(ids)
            assert ix.ntotal == len(xb)
            assert same(ix.search(xq, 10), br.search(xb, xq, 10, id_map=lab))
    assert ix.get_stat("binary_add_flushes") <= 8  # one transfer per reader, not per add
    assert br.same_range(ix.range_search(xq, 120), br.range_search(xb, xq, 120, id_map=lab))
    ix.reset()
    assert ix.ntotal == 0 and np.all(ix.search(xq, 2)[1] == -1)
    ix.add_with_ids(xb[:100], lab[:100])
    assert ix.ntotal == 100 and same(ix.search(xq, 10), br.search(xb[:100], xq, 10, id_map=lab[:100]))


def test_torch_route_equals_host_route(mf):
    import torch

    xb, xq = codes(41, 5000, 256), codes(42, 40, 256)
    ids = np.arange(5000, dtype=np.int64) * 5 + 3
    for with_ids in (False, True):
        ix = mf.index_binary_factory(256, "IDMap,BFlat" if with_ids else "BFlat")
        ix.add_torch(torch.from_numpy(xb).cuda(), torch.from_numpy(ids).cuda() if with_ids else None)
        torch.cuda.synchronize()
        assert ix.ntotal == 5000
        D, I = ix.search_torch(torch.from_numpy(xq).cuda(), 10)
        want = br.search(xb, xq, 10, id_map=ids if with_ids else None)
        assert same((D.cpu().numpy(), I.cpu().numpy()), want) and same(ix.search(xq, 10), want)


# ---- range_search
@pytest.mark.parametrize("idmap", [False, True])
def test_range_search(mf, idmap):
    xb, xq = codes(51, 3000, 64), codes(52, 41, 64)
    xb[[5, 700, 2999]] = xq[3]  # planted duplicates
    xb[64] = xq[40]
    ids = np.random.default_rng(53).permutation(9000)[:3000].astype(np.int64) if idmap else None
    ix = build(mf, 64, xb, ids)
    dist = br.ham(xq, xb)
    lims, D, I = ix.range_search(xq, 0)
    assert lims.tolist() == [0] * 42 and D.size == 0 and I.size == 0
    got = ix.range_search(xq, 1)
    assert br.same_range(got, br.range_search(xb, xq, 1, id_map=ids, dist=dist)) and got[0][-1] == 4
    radius = int(np.quantile(dist, 0.01))
    want = br.range_search(xb, xq, radius, id_map=ids, dist=dist)
    assert want[0][-1] > 100 and br.same_range(ix.range_search(xq, radius), want)
    lab = ids if idmap else np.arange(3000)
    sel = ("batch", lab[::3])
    assert br.same_range(ix.range_search(xq, radius + 2, sel=sel), br.range_search(xb, xq, radius + 2, sel=sel, id_map=ids, dist=dist))
    sel = ("bitmap", bitmap_of(lab[1::2]))
    assert br.same_range(ix.range_search(xq, radius + 2, sel=sel), br.range_search(xb, xq, radius + 2, sel=sel, id_map=ids, dist=dist))
    ix.set_option("binary_stream_cap", 64)  # the hit stream overflows and the scan runs again with the exact size
    assert br.same_range(ix.range_search(xq, radius), want) and ix.get_stat("binary_rescans") > 0
    lims, D, I = ix.range_search(xq[:0], 5)
    assert lims.tolist() == [0]


def test_range_radius_beyond_d_gives_every_row(mf):
    xb, xq = codes(54, 500, 24), codes(55, 17, 24)
    lims, D, I = build(mf, 24, xb).range_search(xq, 25)
    assert np.array_equal(lims, np.arange(18) * 500) and np.array_equal(I, np.tile(np.arange(500), 17))
    assert np.array_equal(D, br.ham(xq, xb).reshape(-1).astype(np.float32)) and D.dtype == np.float32


# ---- reconstruct
def test_reconstruct(mf):
    xb = codes(61, 700, 72)
    ix = build(mf, 72, xb)
    assert np.array_equal(ix.reconstruct(699), xb[699]) and np.array_equal(ix.reconstruct_n(60, 300), xb[60:360])
    assert ix.reconstruct_n(0, 0).shape == (0, 9)
    for call in (lambda: ix.reconstruct(700), lambda: ix.reconstruct(-1), lambda: ix.reconstruct_n(650, 51)):
        with pytest.raises(mf.FaissException, match=r"'ni == 0 \|\| \(i0 >= 0 && i0 \+ ni <= ntotal\)' failed"):
            call()
    ids = np.arange(700, dtype=np.int64) * 2 + 10
    ids[10] = ids[400]  # a duplicate id: the row added last wins
    im = build(mf, 72, xb, ids)
    assert np.array_equal(im.reconstruct(int(ids[3])), xb[3]) and np.array_equal(im.reconstruct(int(ids[400])), xb[400])
    got = im.reconstruct_n(1000, 1)
    assert np.array_equal(got[0], xb[495])
    with pytest.raises(mf.FaissException, match="key not found: 11"):
        im.reconstruct(11)
    with pytest.raises(mf.FaissException, match="key not found: 1001"):
        im.reconstruct_n(1000, 3)


# ---- files
def test_file_round_trip(mf, tmp_path):
    xb, xq = codes(71, 1000, 264), codes(72, 20, 264)
    ids = np.random.default_rng(73).integers(-50, 1 << 45, 1000)
    for desc, lab in (("BFlat", None), ("IDMap,BFlat", ids), ("IDMap2,BFlat", ids)):
        ix = build(mf, 264, xb, lab, desc)
        f = str(tmp_path / (desc.replace(",", "_") + ".bin"))
        mf.write_index_binary(ix, f)
        raw = open(f, "rb").read()
        assert raw == br.write_image(xb, 264, id_map=lab, idmap2=desc.startswith("IDMap2"))  # device -> file equals the model's image
        im = br.parse_image(raw)
        assert np.array_equal(im["codes"], xb) and (lab is None or np.array_equal(im["ids"], lab))
        g = str(tmp_path / "model.bin")
        open(g, "wb").write(br.write_image(xb, 264, id_map=lab, idmap2=desc.startswith("IDMap2")))
        back = mf.read_index_binary(g)  # Python writer -> read_index_binary -> search equals the model
        assert back.ntotal == 1000 and back.d == 264 and back.kind == ix.kind
        assert same(back.search(xq, 10), br.search(xb, xq, 10, id_map=lab))
        with pytest.raises(mf.FaissException, match="not recognized"):
            mf.read_index(f)  # the float reader refuses a binary file
    for cut in (3, 20, 40, len(raw) - 1):
        open(g, "wb").write(raw[:cut])
        with pytest.raises(mf.FaissException, match="truncated"):
            mf.read_index_binary(g)
    open(g, "wb").write(br.write_image(xb, 264, code_size=32))
    with pytest.raises(mf.FaissException, match="code_size = 32"):
        mf.read_index_binary(g)
    open(g, "wb").write(br.write_image(xb, 264, nbytes=33001) + b"\0")
    with pytest.raises(mf.FaissException, match="33001 bytes"):
        mf.read_index_binary(g)
    flat = mf.index_factory(8, "Flat", mf.METRIC_L2)
    flat.add(np.zeros((2, 8), np.float32))
    mf.write_index(flat, g)
    with pytest.raises(mf.FaissException, match="IxF2"):
        mf.read_index_binary(g)  # a float index's fourcc


# ---- factory and refusals
def test_factory_and_refusals(mf):
    for desc in ("BIVF16", "BHNSW8", "BHash4", "IDMap,BIVF16"):
        with pytest.raises(mf.FaissException, match="This index type is not implemented on the MI355X path yet: " + desc):
            mf.index_binary_factory(64, desc)
    with pytest.raises(mf.FaissException, match="could not parse index string Nonsense"):
        mf.index_binary_factory(64, "Nonsense")
    with pytest.raises(mf.FaissException, match="'d % 8 == 0' failed"):
        mf.index_binary_factory(12, "BFlat")
    with pytest.raises(mf.FaissException, match=r"not implemented on the MI355X path yet: .*d = 2056 \(at most 2048 bits\)"):
        mf.index_binary_factory(2056, "BFlat")
    x = codes(81, 4, 64)
    with pytest.raises(mf.FaissException, match="add does not make sense"):
        mf.index_binary_factory(64, "IDMap,BFlat").add(x)
    with pytest.raises(mf.FaissException, match="add_with_ids not implemented for this type of index"):
        mf.index_binary_factory(64, "BFlat").add_with_ids(x, np.arange(4))
    ix = mf.index_binary_factory(64, "BFlat")
    assert ix.is_trained and ix.metric_type == 1 and ix.index is None
    ix.train(x)


# ---- the faiss:: adaptor classes
def test_boundary_driver_binary_mode():
    out = subprocess.run([DRIVER, "binary", "3000", "256", "40", "IDMap,BFlat"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "BINARY OK" in out.stdout
