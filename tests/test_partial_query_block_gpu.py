"""A query block of the d <= 128 coarse-filter scan that is not full (csrc/flat_collect.h collect_qblock_wave): its live tile columns are
spread over the workgroup's four waves, and the columns left over are shared -- a wave runs such a column only on some of the 32-row tiles
of a stage.  Whatever the layout, the scan returns the labels and the distance bits of the exact f32 kernel (prefilter 0), L2 and inner
product, for batch sizes that hit every way the rule can go: a last column with one live query, one column each and one shared, the
headline's last block (272 queries), thirteen columns, sixteen with a ragged end (the full layout), a full block plus one query, 512 + 272,
and two full blocks plus half a column.  A shared column goes wrong by row tile, so one query of EVERY live tile column sits on a planted
cluster of eight rows -- one in each of the four row tiles of the store's first stage and of its last full one -- and under L2 those
eight rows must lead its list.  N = 262 144 + 129 rows: the smallest int8 store, ending inside a stage.  Every case asserts the store
and the kernel that served it, so that none passes on another path."""

import numpy as np
import pytest

L2, IP = 1, 0
KERNEL = "flat_bf16_collect_kernel"
N = 262_144 + 129
BATCHES = [129, 160, 272, 400, 497, 513, 784, 1040]
# one row in each of the four 32-row tiles of a 128-row stage: the first stage, and the last full one (rows 262 144 .. 262 271)
PLANTED = [5, 37, 69, 101, 262_144 + 3, 262_144 + 35, 262_144 + 67, 262_144 + 99]


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss

    return mi355_faiss


@pytest.fixture(scope="module")
def data():
    rs = np.random.RandomState(731)
    xb = rs.rand(N, 128).astype(np.float32)
    xq = rs.rand(max(BATCHES), 128).astype(np.float32)
    centre = (0.1 + 0.8 * rs.rand(128)).astype(np.float32)
    for j, r in enumerate(PLANTED):  # near-copies of the centre, each at a distance of its own, inside the data's range (the int8 store's scale)
        xb[r] = np.clip(centre + (1e-3 * (j + 1)) * rs.randn(128).astype(np.float32), 0.0, 1.0)
    return xb, xq, centre


def _index(mf, metric, xb, prefilter, cl_i8=1):
    ix = mf.index_factory(128, "Flat", metric)
    ix.set_option("prefilter", prefilter)
    ix.set_option("cl_i8", cl_i8)
    for i0 in range(0, len(xb), 1 << 16):
        ix.add(xb[i0 : i0 + (1 << 16)])
    return ix


@pytest.fixture(scope="module")
def indexes(mf, data):
    xb = data[0]
    made = {}

    def get(metric, prefilter, cl_i8=1):
        key = (metric, prefilter, cl_i8)
        if key not in made:
            made[key] = _index(mf, metric, xb, prefilter, cl_i8)
        return made[key]

    return get


def _same(a, b):
    (D1, I1), (D2, I2) = a, b
    return np.array_equal(I1, I2) and np.array_equal(D1.view(np.uint32), D2.view(np.uint32))


def _targets(nq):
    """one query of every live tile column of 32 queries (a position inside the column that changes from column to column)"""
    out = []
    for col in range((nq + 31) // 32):
        q = 32 * col + (7 * col) % 32
        out.append(q if q < nq else 32 * col)
    return out


def _queries(data, nq):
    _, xq, centre = data
    q = xq[:nq].copy()
    t = _targets(nq)
    q[t] = centre
    return q, t


def _search_scan(ix, xq, k, i8=1, **kw):
    r = ix.search(xq, k, **kw)
    assert ix.last_kernel_info()["name"] == KERNEL
    assert ix.get_stat("cl_store_i8") == i8
    return r


def _exact(ix, xq, k, **kw):
    r = ix.search(xq, k, **kw)
    assert ix.last_kernel_info()["name"] != KERNEL
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nq", BATCHES)
def test_batch_sizes(indexes, data, metric, nq):
    xq, targets = _queries(data, nq)
    r8 = _search_scan(indexes(metric, 2), xq, 10)
    if metric == L2:
        for t in targets:
            assert sorted(int(x) for x in r8[1][t][:8]) == PLANTED, "query %d of %d: the planted rows do not lead its list" % (t, nq)
    assert _same(r8, _exact(indexes(metric, 0), xq, 10)), "nq = %d differs from the exact f32 kernel" % nq


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_headline_block_with_32_classes(indexes, data, metric):
    xq, targets = _queries(data, 272)
    r8 = _search_scan(indexes(metric, 2), xq, 32)
    if metric == L2:
        for t in targets:
            assert sorted(int(x) for x in r8[1][t][:8]) == PLANTED
    assert _same(r8, _exact(indexes(metric, 0), xq, 32))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_headline_block_with_selector(indexes, data, metric):
    xq, targets = _queries(data, 272)
    ids = np.arange(0, N, 3, dtype=np.int64)
    r8 = _search_scan(indexes(metric, 2), xq, 10, sel=("batch", ids))
    assert np.all(r8[1] % 3 == 0)
    if metric == L2:
        kept = sorted(r for r in PLANTED if r % 3 == 0)
        for t in targets:
            assert sorted(int(x) for x in r8[1][t][: len(kept)]) == kept
    assert _same(r8, _exact(indexes(metric, 0), xq, 10, sel=("batch", ids)))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_headline_block_on_the_bf16_store(indexes, data, metric):
    xq, targets = _queries(data, 272)
    rb = _search_scan(indexes(metric, 2, 0), xq, 10, i8=0)
    if metric == L2:
        for t in targets:
            assert sorted(int(x) for x in rb[1][t][:8]) == PLANTED
    assert _same(rb, _exact(indexes(metric, 0), xq, 10))
