"""tests/scan_subsample_model.py against checks that do not share its code path: the thinning by the two all-pairs properties that pin the greedy
answer, the voxel outputs as a partition, the hash against values written out by hand.  No GPU."""
import numpy as np
import pytest

import knn_model as km
import scan_subsample_model as sm

CLOUDS = ("uniform", "lattice", "duplicates", "identical", "flat", "collinear", "clusters", "shifted_sphere", "one")


def _extent(p):
    return float((p.max(axis=0) - p.min(axis=0)).max())


def test_the_hash_is_the_splitmix64_finaliser_twice():
    assert sm.mix(sm.GOLDEN) == 0xE220A8397B1DCDAF          # splitmix64's first output from the state 0
    assert sm.thin_key(0, 0) == 0x48218226FF3CD4BF
    assert sm.thin_key(0, 1) == 0xEA8568D2E45FD6CB
    assert sm.thin_key(1, 2 ** 31 - 1) == 0x5C2F1AEF07598188
    assert sm.thin_order(5, priority=[3, -1, 3, -(2 ** 63), 2 ** 63 - 1]) == [3, 1, 0, 2, 4]          # signed, ties by index


@pytest.mark.parametrize("name", CLOUDS)
@pytest.mark.parametrize("seed", [0, 1])
def test_the_greedy_answer_is_independent_and_every_removed_point_has_an_earlier_kept_conflict(name, seed):
    p, (order, d2s) = km.cloud(name)
    p = p[:300]
    ext = _extent(p)
    for r in (0.0, 0.05 * ext, 0.2 * ext, 10.0 * ext, 1.0, np.nextafter(1.0, 2.0)):
        keep, depth = sm.min_distance_thin(p, r, seed=seed)
        a, b = sm.check_thinning(p, r, keep, seed=seed)
        assert a and b, r
        assert 1 <= depth <= len(p) and keep[sm.thin_order(len(p), seed=seed)[0]]
        if r == 0.0:
            assert keep.all() and depth == 1
        if r == 10.0 * ext and ext > 0:
            assert keep.sum() == 1
    # the independent properties (a) and (b) pin the answer: a wrong mask fails one of them
    keep, _ = sm.min_distance_thin(p, 0.2 * ext, seed=seed)
    if not keep.all():
        flipped = keep.copy()
        flipped[np.flatnonzero(~keep)[0]] = True
        assert not sm.check_thinning(p, 0.2 * ext, flipped, seed=seed)[0]          # it conflicts with a kept point: (a) breaks
    flipped = keep.copy()
    flipped[np.flatnonzero(keep)[-1]] = False          # it was kept for having no earlier kept conflict: removed, it breaks (b)
    assert sm.check_thinning(p, 0.2 * ext, flipped, seed=seed) == (True, False)


def test_a_priority_chain_has_the_depth_of_its_length():
    r = 1.0
    p = np.zeros((200, 3))
    p[:, 0] = np.arange(200) * 0.9 * r
    keep, depth = sm.min_distance_thin(p, r, priority=np.arange(200))
    assert np.array_equal(keep, np.arange(200) % 2 == 0) and depth == 200
    assert sm.check_thinning(p, r, keep, priority=np.arange(200)) == (True, True)
    keep_eq, _ = sm.min_distance_thin(p, r, priority=np.zeros(200, np.int64))          # all equal: the ties go by index
    assert np.array_equal(keep_eq, keep)


@pytest.mark.parametrize("name", CLOUDS)
def test_the_voxels_partition_the_points(name):
    p, _ = km.cloud(name)
    p = p[:300]
    ext = _extent(p)
    for h in ([ext, ext / 7.0] if ext > 0 else []) + [1.0, 2.0 ** -30]:
        if ext / h >= 2.0 ** 19 or np.abs(p).max() / h >= 2.0 ** 20:
            with pytest.raises(ValueError):
                sm.voxel_subsample(p, h)
            continue
        v = sm.voxel_subsample(p, h)
        m = v["m"]
        assert int(v["count"].sum()) == len(p) and sorted(set(v["voxel"])) == list(range(m))
        assert np.array_equal(np.bincount(v["voxel"], minlength=m), v["count"])
        assert (np.diff(v["first"]) > 0).all()          # numbered by first member
        for row in range(m):
            members = np.flatnonzero(v["voxel"] == row)
            assert v["first"][row] == members[0] and v["nearest"][row] in members and v["first"][row] <= v["nearest"][row]
            cells = np.floor((p[members] - 0.0) / h)
            assert (cells == cells[0]).all()
        firsts = np.floor(p[v["first"]] / h)
        assert len({tuple(c) for c in firsts}) == m          # no voxel twice


def test_the_centroid_sum_is_chunked_at_256_members():
    x = np.random.default_rng(0).random(513) * 2.0 ** np.random.default_rng(1).integers(-20, 20, 513)
    want = (float(np.cumsum(x[:256])[-1]) + float(np.cumsum(x[256:512])[-1])) + x[512]
    assert sm.serial_chunk_sum(x) == want
    assert sm.serial_chunk_sum(x[:256]) == float(np.cumsum(x[:256])[-1])
    assert sm.serial_chunk_sum(np.array([-0.0])) == 0.0 and not np.signbit(sm.serial_chunk_sum(np.array([-0.0])))
