"""ops.voxel_subsample and ops.min_distance_thin (csrc/scansub.hip) against the numpy restatement tests/scan_subsample_model.py:
every index, and every fp64 value as int64 bits, whatever the grid resolution, and again on a rerun.  No tolerance appears here."""
import functools

import numpy as np
import pytest
import torch

import knn_model as km
import scan_subsample_model as sm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RESOLUTIONS = (0, 1, 2, 7, 64, None)
CLOUDS = sorted(km.CLOUDS)
VOXEL_KEYS = ("voxel", "count", "first", "nearest", "centroid")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _box(p):
    lo, hi = p.min(axis=0), p.max(axis=0)
    return lo, float((hi - lo).max())


# ---- voxel grid ------------------------------------------------------------------------------------------------------------------------
def _voxel(p, h, origin=(0.0, 0.0, 0.0)):
    from dgnn_amd import ops
    out = ops.voxel_subsample(torch.from_numpy(np.array(p)).to(DEV), h, origin=origin)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _assert_voxels(got, want, n):
    m = want["m"]
    assert got["m"] == m and sorted(got) == sorted(want)
    for key in VOXEL_KEYS:
        assert got[key].dtype == want[key].dtype == (np.float64 if key == "centroid" else np.int32), key
        assert got[key].shape == want[key].shape == {"voxel": (n,), "centroid": (m, 3)}.get(key, (m,)), key
    for key in ("voxel", "count", "first", "nearest"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(_bits(got["centroid"]), _bits(want["centroid"]))


def _voxel_case(p, h, origin=(0.0, 0.0, 0.0)):
    got = _voxel(p, h, origin)
    _assert_voxels(got, sm.voxel_subsample(p, h, origin), len(p))
    return got


@pytest.mark.parametrize("name", CLOUDS)
def test_voxels_equal_the_model(name):
    p, _ = km.cloud(name)
    lo, ext = _box(p)
    one = _voxel_case(p, 2.0 * ext if ext > 0 else 1.0, lo)          # everything in one voxel
    assert one["m"] == 1 and one["count"][0] == len(p) and one["first"][0] == 0
    if ext > 0:
        _voxel_case(p, ext, lo)                       # the extent: the far faces of the box are ON a voxel face
        _voxel_case(p, ext / 7.0, lo)
        _voxel_case(p, ext / 7.0, lo + 0.37 * ext)          # a non-zero origin inside the cloud: negative voxel coordinates
        alone = _voxel_case(p, ext * 2.0 ** -19, lo)          # as fine as the key allows: every distinct point alone
        assert alone["m"] == len(np.unique(np.floor((p - lo) / (ext * 2.0 ** -19)), axis=0))
        mid = p - (lo + 0.5 * (p.max(axis=0) - lo))          # straddling 0: floor and truncation differ
        got = _voxel_case(mid, ext / 7.0)
        assert (np.floor(mid / (ext / 7.0)) < 0).any() and got["m"] > 1
    if np.abs(p).max() < 2.0 ** 19:
        _voxel_case(p, 1.0)          # the lattice's spacing exactly: its points sit on voxel faces
        _voxel_case(p, 1.0, (0.125, -0.25, 0.5))


def test_the_lattice_at_its_spacing_has_one_point_per_voxel():
    p, _ = km.cloud("lattice")
    got = _voxel_case(p, 1.0)
    assert got["m"] == 125 and np.array_equal(got["first"], np.arange(125)) and np.array_equal(got["nearest"], np.arange(125))
    assert np.array_equal(_bits(got["centroid"]), _bits(p))
    assert _voxel_case(p, 2.0)["m"] == 27


def test_voxels_of_257_and_513_members_cross_the_chunks_of_the_centroid_sum():
    rng = np.random.default_rng(7)
    heavy = [rng.random((cnt, 3)) * 2.0 ** rng.integers(-30, 0, (cnt, 3)) + base for cnt, base in ((257, 0.0), (513, 2.0), (256, 4.0), (64, 6.0), (65, 8.0))]
    p = np.concatenate(heavy + [10.0 + 3.0 * rng.random((40, 3))])
    p = np.ascontiguousarray(p[rng.permutation(len(p))])
    got = _voxel_case(p, 1.0)
    assert {257, 513, 256, 64, 65} <= set(got["count"].tolist())
    v = int(np.flatnonzero(got["count"] == 513)[0])
    members = np.flatnonzero(got["voxel"] == v)
    plain = np.cumsum(p[members, 0])[-1] / 513.0
    assert got["centroid"][v, 0] == sm.serial_chunk_sum(p[members, 0]) / 513.0
    print("513 members: chunked centroid x %r, one serial sum %r" % (got["centroid"][v, 0], plain))


def test_no_points_and_one_point_and_a_rerun():
    got = _voxel(np.zeros((0, 3)), 1.0)
    assert got["m"] == 0 and all(got[k].shape == ((0, 3) if k == "centroid" else (0,)) for k in VOXEL_KEYS)
    p, _ = km.cloud("one")
    one = _voxel_case(p, 0.25)
    assert one["m"] == 1 and np.array_equal(_bits(one["centroid"]), _bits(p)) and one["nearest"][0] == 0
    p, _ = km.cloud("uniform")
    a, b = _voxel(p, 1.0 / 7.0), _voxel(p, 1.0 / 7.0)
    for key in VOXEL_KEYS:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_voxel_refusals():
    p = np.array([[0.5, 0.25, 0.125], [3.0, -2.0, 1.0]])
    for h in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel size"):
            _voxel(p, h)
    bad = p.copy()
    bad[1, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        _voxel(bad, 1.0)
    h = 0.5
    for edge, inside in ((2.0 ** 20 * h, np.nextafter(2.0 ** 20 * h, 0.0)), (-(2.0 ** 20) * h, -(2.0 ** 20) * h + h)):
        for a in range(3):
            q = p.copy()
            q[0, a] = edge
            with pytest.raises(ValueError, match=r"2\^20"):
                _voxel(q, h)
            q[0, a] = inside
            got = _voxel_case(q, h)
            assert got["m"] == 2
    with pytest.raises(ValueError, match=r"2\^20"):
        _voxel(p, h, origin=(0.0, 2.0 ** 20, 0.0))


# ---- thinning --------------------------------------------------------------------------------------------------------------------------
def _thin(p, r, R=None, priority=None, seed=0):
    from dgnn_amd import ops
    pr = None if priority is None else torch.from_numpy(np.asarray(priority, dtype=np.int64)).to(DEV)
    keep, stats = ops.min_distance_thin(torch.from_numpy(np.array(p)).to(DEV), r, priority=pr, seed=seed, grid_resolution=R, return_stats=True)
    assert keep.dtype == torch.bool and tuple(keep.shape) == (len(p),)
    return keep.cpu().numpy(), stats


@functools.lru_cache(maxsize=None)
def _model(name, r, seed):
    p, _ = km.cloud(name)
    keep, depth = sm.min_distance_thin(p, r, seed=seed)
    keep.setflags(write=False)
    return keep, depth


def _every_resolution(p, r, want, depth, priority=None, seed=0):
    first = None
    for R in RESOLUTIONS:
        keep, stats = _thin(p, r, R, priority, seed)
        assert np.array_equal(keep, want), R
        assert stats["n_kept"] == int(keep.sum()) == int(want.sum())
        assert 1 <= stats["rounds"] <= depth + 1, (R, stats, depth)
        assert stats["candidates"] >= len(p)          # every point reads its own record at least
        first = keep if first is None else first
    again, _ = _thin(p, r, None, priority, seed)
    assert again.tobytes() == first.tobytes()          # the default on a rerun against no grid, in every byte
    assert sm.check_thinning(p, r, again, priority=priority, seed=seed) == (True, True)          # from the device's mask alone
    return first


def _radii(p):
    _, ext = _box(p)
    return (0.0, 0.05 * ext, 0.2 * ext, 10.0 * ext) if ext > 0 else (0.0, 1.0)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", CLOUDS)
def test_thinning_equals_the_model_at_every_resolution(name, seed):
    p, _ = km.cloud(name)
    _, ext = _box(p)
    order = sm.thin_order(len(p), seed=seed)
    for r in _radii(p):
        want, depth = _model(name, r, seed)
        keep = _every_resolution(p, r, want, depth, seed=seed)
        if r == 0.0:
            assert keep.all()          # duplicates included
        elif r == 10.0 * ext or ext == 0.0:
            assert np.array_equal(np.flatnonzero(keep), [order[0]])          # exactly one: the first in the order


def test_a_distance_equal_to_the_radius_is_no_conflict():
    p, _ = km.cloud("lattice")
    want, depth = sm.min_distance_thin(p, 1.0)
    assert want.all() and depth == 1
    _every_resolution(p, 1.0, want, depth)
    above = float(np.nextafter(1.0, 2.0))
    want, depth = sm.min_distance_thin(p, above)
    assert not want.all()
    _every_resolution(p, above, want, depth)


def test_a_priority_chain_takes_many_rounds_and_equal_priorities_go_by_index():
    r = 1.0
    p = np.zeros((200, 3))
    p[:, 0] = np.arange(200) * 0.9 * r
    chain = np.arange(200, dtype=np.int64)
    want, depth = sm.min_distance_thin(p, r, priority=chain)
    assert depth == 200 and np.array_equal(want, np.arange(200) % 2 == 0)
    _every_resolution(p, r, want, depth, priority=chain)
    _, stats = _thin(p, r, 7, chain)
    assert stats["rounds"] > 50          # the many-rounds path, several host read-backs
    for pr in (np.zeros(200, np.int64), np.full(200, -(2 ** 63)), np.full(200, 2 ** 63 - 1)):
        want_eq, depth_eq = sm.min_distance_thin(p, r, priority=pr)
        assert np.array_equal(want_eq, want)
        _every_resolution(p, r, want_eq, depth_eq, priority=pr)
    q, _ = km.cloud("uniform")
    pr = np.random.default_rng(3).integers(-5, 5, len(q))          # signed, many ties
    want, depth = sm.min_distance_thin(q, 0.1, priority=pr)
    _every_resolution(q, 0.1, want, depth, priority=pr)


def test_no_points_and_thinning_refusals():
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    for R in (0, 3, None):
        keep, stats = _thin(np.zeros((0, 3)), 0.5, R)
        assert keep.shape == (0,) and stats == dict(n_kept=0, rounds=0, candidates=0)
    p, _ = km.cloud("flat")
    for r in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            _thin(p, r, 2)
    bad = p.copy()
    bad[17, 1] = float("inf")
    for R in (0, 2):
        with pytest.raises(ValueError, match="non-finite"):
            _thin(bad, 0.1, R)
    with pytest.raises(ValueError, match="priorities"):
        _thin(p, 0.1, 2, priority=np.arange(3))
    with pytest.raises(DgnnError):
        _thin(p, 0.1, 1025)
    assert [ops.default_thin_resolution(e, r) for e, r in ((1.0, 0.01), (1.0, 0.1), (1.0, 2.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1e-9))] == [25, 2, 1, 1, 1, 512]
