"""The statistical claims of the cell-label sampler, on the numpy model: they are about the definition, not the device, and
tests/test_gpu_cell_labels.py holds the device to this model bit for bit.  Fixed seeds: nothing here can flake."""
import numpy as np
import pytest

import cell_labels_model as cl
import mesh_contains_model as mc

K = 65536
SEEDS = [0, 1, 7]
UNIT_V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
UNIT_T = np.array([[0, 1, 2, 3]], dtype=np.int32)


@pytest.mark.parametrize("seed", SEEDS)
def test_barycentrics_lie_in_the_unit_tet(seed):
    b = cl.barycentrics(seed, 1, K)
    assert b.shape == (K, 3) and b.dtype == np.float64
    assert (b >= 0).all()
    # the three folded values are each one rounding of an exact value whose sum is <= 1: their fp64 sum exceeds 1 by one rounding at most
    assert ((b[:, 0] + b[:, 1]) + b[:, 2]).max() <= 1 + 2.0 ** -52
    assert 1 - b.sum(axis=1).min() > 0.5          # and they are not all pushed onto the slanted face


@pytest.mark.parametrize("seed", SEEDS)
def test_samples_are_uniform_on_the_unit_tet(seed):
    """on the unit tet the point is (s, t, u) itself.  P(x < 0.5) = 1 - (1/2)^3 = 0.875 (binomial: sigma = sqrt(p q / k)); a coordinate has
    mean 1/4 and variance 3/80 (sigma of the mean = sqrt(3 / 80 / k)).  5 sigma each."""
    p = cl.sample_points(UNIT_V, UNIT_T, K, seed)
    assert np.array_equal(p, cl.barycentrics(seed, 1, K))
    share = (p[:, 0] < 0.5).mean()
    print("seed %d: share x < 0.5 = %.5f, means %s, E[x^2] %s" % (seed, share, p.mean(axis=0), (p * p).mean(axis=0)))
    assert abs(share - 0.875) <= 5 * np.sqrt(0.875 * 0.125 / K)
    assert (np.abs(p.mean(axis=0) - 0.25) <= 5 * np.sqrt(3 / 80 / K)).all()


def test_the_counter_walks_through_tets_and_offsets():
    """tet t of a call with tet_offset o draws what tet 0 of a call with tet_offset o + t draws"""
    v = np.concatenate([UNIT_V, UNIT_V + 2.0])
    tets = np.array([[0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 2, 3]], dtype=np.int32)
    p = cl.sample_points(v, tets, 37, 3).reshape(3, 37, 3)
    assert np.array_equal(p[2], cl.sample_points(v, tets[:1], 37, 3, tet_offset=2))
    assert not np.array_equal(p[2], p[0])
    big = cl.sample_points(v, tets[:1], 5, 3, tet_offset=2 ** 40)
    assert not np.array_equal(big, cl.sample_points(v, tets[:1], 5, 3, tet_offset=0)) and ((0 <= big) & (big <= 1)).all()


def test_volume_fraction_of_the_unit_tet_in_a_cube():
    """the cube [-3, 0.5]^3 cuts the corner tets x, y, z >= 0.5 off the unit tet: 1 - 3 (1/2)^3 = 0.625 of it is inside"""
    count, inside, outside, n_disagree = cl.labels(*mc.cube(-3.0, 0.5), UNIT_V, UNIT_T, K, 0)
    print("inside %.5f (exact 0.625), n_disagree %d" % (inside[0], n_disagree))
    assert count.dtype == np.int32 and inside[0] == count[0] / K and outside[0] == (K - count[0]) / K and inside[0] + outside[0] == 1.0
    assert abs(inside[0] - 0.625) <= 5 * np.sqrt(0.625 * 0.375 / K)
