"""Who trains with kmeans_train (csrc/clustering.hip) and what each caller must keep: the HNSW-quantiser branch of IVF<n>,Flat (k-means on a
local Flat L2 index, the centroids then inserted into the graph) bit for bit against the oracle, and its refusal to take centroids twice;
the coded kinds' coarse training (spherical under inner product, with the index's tuning) bit for bit against what IVF<n>,Flat learns from
the same rows; PQ<M>'s per-sub-space training repeatable and leaving no device memory behind."""
import gc

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
L2, IP = orc.METRIC_L2, orc.METRIC_INNER_PRODUCT


@pytest.fixture(scope="module")
def mf():
    import mi355_faiss

    return mi355_faiss


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_hnsw_quantiser_training_bit_identical_to_oracle(mf):
    xb = orc.synth_clustered(6000, 32, 7, n_centers=64, sigma=0.15)
    o = orc.Index(32, "IVF16_HNSW8,Flat", L2)
    o.train(xb)
    g = mf.index_factory(32, "IVF16_HNSW8,Flat", L2)
    assert not g.is_trained and g.nlist == 16
    g.train(xb)
    assert g.is_trained and g.quantizer.ntotal == 16 and g.quantizer.kind == mf.KIND_HNSW
    got = g.ivf_centroids()
    assert np.array_equal(_bits(got), _bits(o.ivf_centroids()))
    with pytest.raises(mf.FaissException, match="the HNSW coarse quantizer already holds centroids"):
        g.ivf_set_centroids(got)
    assert np.array_equal(_bits(g.ivf_centroids()), _bits(got))  # (the refusal changed nothing)


@pytest.fixture(scope="module")
def ip_rows_and_centroids(mf):
    xb = orc.synth_clustered(3000, 16, 3, n_centers=8, sigma=0.15)
    flat = mf.index_factory(16, "IVF8,Flat", IP)
    flat.train(xb)
    cent = flat.ivf_centroids()
    cent.setflags(write=False)
    return xb, cent


@pytest.mark.parametrize("desc", ["IVF8,PQ4", "IVF8,SQ8"])
def test_coded_kinds_learn_ivfflat_centroids_under_inner_product(mf, ip_rows_and_centroids, desc):
    xb, cent = ip_rows_and_centroids
    # spherical k-means keeps unit-norm centroids (renorm_l2's f32 chain: within a few ulp of 1) -- so the L2 variant cannot pass by accident
    assert np.abs(np.linalg.norm(cent.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    g = mf.index_factory(16, desc, IP)
    assert not g.is_trained and g.nlist == 8
    g.train(xb)
    assert g.is_trained and g.quantizer.ntotal == 8
    assert np.array_equal(_bits(g.ivf_centroids()), _bits(cent))


def test_pq_training_repeatable_and_leaves_no_device_memory(mf):
    xb = np.random.default_rng(5).standard_normal((600, 16)).astype(np.float32)
    gc.collect()  # (garbage of earlier tests that holds an index goes now, not between two readings)
    keeper = mf.index_factory(8, "Flat", L2)
    before = keeper.get_stat("device_bytes_live")
    ix = mf.index_factory(16, "PQ4", L2)
    ix.train(xb)
    first = ix.pq_centroids()
    assert ix.is_trained and first.shape == (4, 256, 4)
    ix.train(xb)  # (still empty: training again is allowed)
    assert np.array_equal(_bits(ix.pq_centroids()), _bits(first))
    assert keeper.get_stat("device_bytes_live") > before  # (the codebooks)
    del ix
    gc.collect()
    assert keeper.get_stat("device_bytes_live") == before
