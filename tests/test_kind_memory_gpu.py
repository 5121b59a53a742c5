"""What every index kind besides Flat holds on the device (csrc/dev_mem.h: the stores that keep their contents as they grow, the
code stores remove_ids swaps, the parameter blocks): per kind, at d = 32, rows are added in two halves of 3000 (HNSW: 2000) so that every
row-counted store outgrows its first 4096 rows -- and the HNSW buffers their first 4096 bytes many times -- and
  * reconstruct_n over the first half reads the same BITS after the growth as before it (the prefix a growth has to keep);
  * the search equals the kind's own reference, labels equal and distances as bit patterns, as in the kind's own test file: the oracle for
    the Flat-backed kinds, tests/pq_reference.py, tests/ivfpq_reference.py, tests/sq_reference.py, tests/hnswsq_reference.py,
    tests/refine_reference.py, tests/pretransform_reference.py and tests/binary_reference.py for the others.  Parameters both sides share
    (centroids, codebooks, ranges) are set through the accessors, as those files do; PCA and the HNSW,SQ8 range are trained on the device;
  * where the kind serves remove_ids, 500 random ids go and the search equals the reference of the survivors (the code stores and the
    IVF,Flat rows are gathered into a fresh allocation there);
  * when the index is freed, statistic device_bytes_live, read through an index that stays alive, is back where it started.
The binary kinds follow the same sequence at 256 bits, with one reset() between the first add and the two that count, and read the counter
through IndexBinary.get_stat."""

import gc

import numpy as np
import pytest

import binary_reference as bnr
import hnswsq_reference as hsr
import ivfpq_reference as ivr
import pq_reference as pqr
import pretransform_reference as ptr
import refine_reference as rfr
import remove_reference as rr
import sq_reference as sqr
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT
D, NQ, K, NLIST, NPROBE, EFS = 32, 64, 10, 64, 8, 64


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss

    return mi355_faiss


@pytest.fixture
def live(mf):
    """reads device_bytes_live through a keeper index that outlives the index under test"""
    gc.collect()  # (garbage of earlier tests that holds an index goes now, not between two readings)
    keeper = mf.index_factory(8, "Flat", L2)
    return lambda: keeper.get_stat("device_bytes_live")


def _same(got, want, what):
    (Dg, Ig), (Dr, Ir) = got, want
    assert np.array_equal(Ig, Ir), f"{what}: labels differ in {(Ig != Ir).sum()} slots"
    assert np.array_equal(Dg.view(np.uint32), Dr.view(np.uint32)), f"{what}: distances differ in {(Dg != Dr).sum()} slots"


def _data(seed, n):
    """rows, queries, 64 of the rows as coarse centroids, external ids whose first half is a permutation of 0 .. n/2 - 1 (reconstruct_n
    over the first half needs every key of the range), the 500 ids that go"""
    rng = np.random.default_rng(seed)
    xb = rng.standard_normal((n, D)).astype(np.float32)
    xq = rng.standard_normal((NQ, D)).astype(np.float32)
    cent = xb[rng.permutation(n)[:NLIST]].copy()
    ids = np.concatenate([rng.permutation(n // 2), n // 2 + rng.permutation(n - n // 2)]).astype(np.int64)
    gone = np.sort(rng.permutation(n)[:500]).astype(np.int64)
    return rng, xb, xq, cent, ids, gone


class Case:
    """one kind: the device index, and the reference's answer for the rows `keep` (positions in arrival order) that are still there"""

    n, kw, removes = 6000, {}, True

    def __init__(self, mf, desc, metric, seed):
        self.mf, self.desc, self.metric, self.mapped = mf, desc, metric, desc.startswith("IDMap")
        self.rng, self.xb, self.xq, self.cent, self.ids, self.gone = _data(seed, self.n)
        if not self.mapped:
            self.ids = np.arange(self.n, dtype=np.int64)

    def add(self, ix, lo, hi):
        ix.add_with_ids(self.xb[lo:hi], self.ids[lo:hi]) if self.mapped else ix.add(self.xb[lo:hi])

    def after_add(self, lo, hi):
        pass

    def first_half(self, ix):
        return ix.reconstruct_n(0, self.n // 2)


class IvfFlat(Case):
    kw = dict(nprobe=NPROBE)

    def build(self):
        ix = self.mf.index_factory(D, self.desc, self.metric)
        ix.ivf_set_centroids(self.cent)
        ix.set_option("ivf_mfma", 0)  # (the scanner's arithmetic for inner product too, as tests/test_flat_memory_gpu.py compares it)
        return ix

    def expect(self, keep):  # (IVF,Flat keeps the stored ids of the survivors: the arrival numbers)
        o = orc.Index(D, self.desc, self.metric)
        o.ivf_set_centroids(self.cent)
        o.add_with_ids(self.xb[keep], self.ids[keep])
        return o.search(self.xq, K, nprobe=NPROBE)


class Pq(Case):
    def build(self):
        self.cb = pqr.synthetic_codebooks(self.rng, 8, D // 8)
        self.codes = pqr.encode(self.cb, self.xb)
        ix = self.mf.index_factory(D, self.desc, self.metric)
        ix.pq_set_centroids(self.cb)
        return ix

    def expect(self, keep):  # (bare: the survivors are numbered anew)
        return pqr.search(self.cb, self.codes[keep], self.xq, K, self.metric, labels=self.ids[keep] if self.mapped else None)


class Sq(Case):
    def build(self):
        self.vmin, self.vdiff = sqr.train_range(self.xb)
        self.codes = sqr.encode(self.vmin, self.vdiff, self.xb)
        ix = self.mf.index_factory(D, self.desc, self.metric)
        ix.sq_set_trained(self.vmin, self.vdiff)
        return ix

    def expect(self, keep):
        return sqr.sq_search(self.metric, self.vmin, self.vdiff, self.codes[keep], self.xq, K)


class IvfCoded(Case):
    """IVF64,PQ8 | IVF64,SQ8: the model's lists; after remove_ids every list as FAISS's swap loop leaves it (tests/remove_reference.py)"""

    kw = dict(nprobe=NPROBE)

    def build(self):
        ix = self.mf.index_factory(D, self.desc, self.metric)
        ix.ivf_set_centroids(self.cent)
        if "PQ" in self.desc:
            self.cb = pqr.synthetic_codebooks(self.rng, 8, D // 8)
            ix.pq_set_centroids(self.cb)
            self.lists = ivr.build_lists(self.metric, self.cent, self.cb, self.xb)
        else:
            of_row, _ = sqr.assign(self.metric, self.cent, self.xb)
            self.vmin, self.vdiff = sqr.train_range(sqr.residuals(self.cent, self.xb, of_row))
            ix.sq_set_trained(self.vmin, self.vdiff)
            self.lists = sqr.build_lists(self.metric, self.cent, self.vmin, self.vdiff, self.xb)
        return ix

    def expect(self, keep):
        lists = self.lists
        if len(keep) < self.n:
            orders, new_ids, removed, _ = rr.remove_lists([l[0] for l in lists], ("batch", self.gone))
            assert removed == self.n - len(keep)
            lists = [(new_ids[l], lists[l][1][orders[l]]) for l in range(NLIST)]
        if "PQ" in self.desc:
            return ivr.search(self.metric, self.cent, self.cb, lists, self.xq, K, NPROBE)
        return sqr.ivf_search(self.metric, self.cent, self.vmin, self.vdiff, lists, self.xq, K, NPROBE)


class Hnsw(Case):
    """HNSW16 | HNSW16,SQ8 in the deterministic build order (one build wave), the reference fed the same two chunks"""

    n, kw, removes = 4000, dict(efSearch=EFS), False

    def build(self):
        ix = self.mf.index_factory(D, self.desc, self.metric)
        ix.set_option("hnsw_build_waves", 1)
        if "SQ8" in self.desc:
            ix.train(self.xb)
            self.model = hsr.Model(D, 16, self.metric, self.xb)
        else:
            self.model = orc.Index(D, self.desc, self.metric)
        return ix

    def after_add(self, lo, hi):
        self.model.add(self.xb[lo:hi])

    def expect(self, keep):
        if "SQ8" in self.desc:
            assert hsr.codes_are_distinct(self.model.codes), "the parity needs pairwise distinct code rows"
        return self.model.search(self.xq, K, efSearch=EFS)


class IvfSqRefined(Case):
    kw, removes = dict(nprobe=NPROBE), False

    def build(self):
        ix = self.mf.index_factory(D, self.desc, self.metric)
        of_row, _ = sqr.assign(self.metric, self.cent, self.xb)
        vmin, vdiff = sqr.train_range(sqr.residuals(self.cent, self.xb, of_row))
        ix.refine_base.ivf_set_centroids(self.cent)
        ix.refine_base.sq_set_trained(vmin, vdiff)
        ix.k_factor = 4
        self.model = rfr.Model("IVFSQ", self.metric, D, cent=self.cent, vmin=vmin, vdiff=vdiff)
        self.model.add(self.xb)
        return ix

    def expect(self, keep):
        return self.model.search(self.xq, K, 4, nprobe=NPROBE)


class PcaIvfFlat(Case):
    """PCA16,IVF64,Flat: PCA and centroids trained on the device; the oracle's IVF64,Flat at d = 16 with those centroids over the rows and
    queries the model transforms (tests/pretransform_reference.py).  The wrapper refuses reconstruct (no reverse transform): the first
    half is read from its sub-index, whose rows are the ones that grow"""

    kw = dict(nprobe=NPROBE)

    def build(self):
        ix = self.mf.index_factory(D, self.desc, self.metric)
        ix.train(self.xb)
        A, b = ix.pretransform_get_linear(0)
        chain = [dict(type=ptr.VT_LINEAR, A=A, b=b)]
        self.yb, self.yq = ptr.apply_chain(chain, self.xb), ptr.apply_chain(chain, self.xq)
        self.sub_cent = ix.pretransform_sub.ivf_centroids()
        return ix

    def first_half(self, ix):
        return ix.pretransform_sub.reconstruct_n(0, self.n // 2)

    def expect(self, keep):
        o = orc.Index(16, "IVF64,Flat", self.metric)
        o.ivf_set_centroids(self.sub_cent)
        o.add_with_ids(self.yb[keep], self.ids[keep])
        return o.search(self.yq, K, nprobe=NPROBE)


CASES = [(IvfFlat, "IVF64,Flat", m) for m in (L2, IP)] + [(Pq, "PQ8", m) for m in (L2, IP)] + [(IvfCoded, "IVF64,PQ8", m) for m in (L2, IP)]
CASES += [(Sq, "SQ8", m) for m in (L2, IP)] + [(IvfCoded, "IVF64,SQ8", m) for m in (L2, IP)]
CASES += [(Hnsw, "HNSW16", m) for m in (L2, IP)] + [(Hnsw, "HNSW16,SQ8", m) for m in (L2, IP)]
CASES += [(Pq, "IDMap,PQ8", L2), (IvfSqRefined, "IVF64,SQ8,RFlat", L2), (PcaIvfFlat, "PCA16,IVF64,Flat", L2)]


@pytest.mark.parametrize("cls,desc,metric", CASES, ids=[f"{c[1]}-{'L2' if c[2] == L2 else 'IP'}" for c in CASES])
def test_kind_grows_keeps_its_prefix_and_leaves_nothing_behind(mf, live, cls, desc, metric):
    before = live()
    c = cls(mf, desc, metric, 100 + len(desc) + metric)
    half = c.n // 2
    ix = c.build()
    assert ix.is_trained
    c.add(ix, 0, half)
    c.after_add(0, half)
    first = c.first_half(ix)
    assert live() > before
    c.add(ix, half, c.n)  # (beyond the stores' first capacity: every one of them grows)
    c.after_add(half, c.n)
    assert ix.ntotal == c.n
    assert np.array_equal(c.first_half(ix).view(np.uint32), first.view(np.uint32)), "the first half reads differently after the growth"
    _same(ix.search(c.xq, K, **c.kw), c.expect(np.arange(c.n)), desc)
    if c.removes:
        assert ix.remove_ids(("batch", c.gone)) == 500 and ix.ntotal == c.n - 500
        _same(ix.search(c.xq, K, **c.kw), c.expect(np.nonzero(~np.isin(c.ids, c.gone))[0]), desc + " after remove_ids")
    del ix
    assert live() == before


@pytest.mark.parametrize("desc", ["BFlat", "IDMap,BFlat"])
def test_binary_grows_keeps_its_prefix_and_leaves_nothing_behind(mf, desc):
    bits, n, half = 256, 6000, 3000
    rng = np.random.default_rng(7 + len(desc))
    bb = rng.integers(0, 256, (n, bits // 8), dtype=np.uint8)
    bq = rng.integers(0, 256, (NQ, bits // 8), dtype=np.uint8)
    bq[0] = bb[half + 5]
    mapped = desc.startswith("IDMap")
    ids = np.concatenate([rng.permutation(half), half + rng.permutation(n - half)]).astype(np.int64) if mapped else None

    def add(ix, lo, hi):
        ix.add_with_ids(bb[lo:hi], ids[lo:hi]) if mapped else ix.add(bb[lo:hi])

    gc.collect()
    keeper = mf.index_binary_factory(8, "BFlat")
    before = keeper.get_stat("device_bytes_live")
    ix = mf.index_binary_factory(bits, desc)
    add(ix, 0, half)
    first = ix.reconstruct_n(0, half)  # (small adds wait in pinned memory: a reader brings them to the device)
    assert np.array_equal(first, bb[np.argsort(ids[:half])] if mapped else bb[:half])  # (under IDMap the keys are the external ids)
    assert keeper.get_stat("device_bytes_live") > before
    ix.reset()  # (empty again, its stores kept)
    assert ix.ntotal == 0
    add(ix, 0, half)
    assert np.array_equal(ix.reconstruct_n(0, half), first)
    add(ix, half, n)  # (beyond the 4096 rows of the first allocation: all three stores grow)
    assert ix.ntotal == n
    assert np.array_equal(ix.reconstruct_n(0, half), first), "the first half reads differently after the growth"
    Dg, Ig = ix.search(bq, K)
    Dr, Ir = bnr.search(bb, bq, K, id_map=ids)
    assert np.array_equal(Ig, Ir) and np.array_equal(Dg, Dr), desc + ": results differ from the CPU model"
    assert Dg[0, 0] == 0
    del ix
    assert keeper.get_stat("device_bytes_live") == before
