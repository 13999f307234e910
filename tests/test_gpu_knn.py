"""ops.knn and the scan operations on it (csrc/knn.hip) against the numpy restatement tests/knn_model.py: every index and every
fp64 value bit for bit, whatever the grid resolution, and again on a rerun.  No tolerance appears here."""
import functools

import numpy as np
import pytest
import torch

import knn_model as km

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RESOLUTIONS = (0, 1, 2, 7, 64, None)
KS = (1, 2, 16, 63, 64)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).to(DEV)


def _knn(p, k, R, q=None, **kw):
    from dgnn_amd import ops
    out = ops.knn(_dev(p), k, queries=_dev(q), grid_resolution=R, **kw)
    return tuple(o.cpu().numpy() if isinstance(o, torch.Tensor) else o for o in out)


def _assert_rows(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[0].shape == want[0].shape == got[1].shape
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(_bits(got[1]), _bits(want[1]))


def _every_resolution(p, k, want, q=None):
    first = None
    for R in RESOLUTIONS:
        got = _knn(p, k, R, q)
        _assert_rows(got, want)
        first = first or got
    _assert_rows(_knn(p, k, None, q), first)          # a rerun, and the default against no grid, in every byte


def test_the_default_resolution_is_the_models():
    from dgnn_amd import ops
    for n in (0, 1, 2, 15, 16, 17, 100, 1500, 150000, 10 ** 6, 10 ** 8):
        assert ops.default_knn_resolution(n) == km.default_resolution(n) >= 1


@pytest.mark.parametrize("name", sorted(km.CLOUDS))
def test_points_as_their_own_queries_equal_the_model_at_every_resolution(name):
    p, ordered = km.cloud(name)
    for k in KS:
        _every_resolution(p, k, km.knn(p, k, ordered=ordered))


@pytest.mark.parametrize("k", KS)
def test_a_row_that_the_points_just_fill_or_just_miss(k):
    for n in (k, k + 1):          # n = k: the last column is the pad; n = k + 1: every row is just full
        p = km.small(n, seed=n)
        want = km.knn(p, k)
        assert (want[0][:, -1] == -1).all() == (n == k)
        _every_resolution(p, k, want)


@pytest.mark.parametrize("name", sorted(km.CLOUDS))
def test_separate_queries_equal_the_model_at_every_resolution(name):
    p, _ = km.cloud(name)
    q, ordered = km.cloud_queries(name)          # on points exactly, inside the box, 100 extents outside it
    for k in (1, 16, 64):
        _every_resolution(p, k, km.knn(p, k, q, ordered=ordered), q)


def test_bad_k_and_non_finite_coordinates_are_refused():
    from dgnn_amd import ops
    p, _ = km.cloud("uniform")
    for k in (0, 65, -1):
        with pytest.raises(ValueError):
            ops.knn(_dev(p), k)
    for bad in (np.nan, np.inf):
        broken = np.array(p)
        broken[17, 1] = bad
        for R in (0, None):
            with pytest.raises(ValueError, match="non-finite"):
                ops.knn(_dev(broken), 4, grid_resolution=R)
            with pytest.raises(ValueError, match="non-finite"):
                ops.knn(_dev(p), 4, queries=_dev(broken[:40]), grid_resolution=R)
    idx, d2 = ops.knn(_dev(p), 4)          # the library is sound after a refusal
    _assert_rows((idx.cpu().numpy(), d2.cpu().numpy()), km.knn(p, 4, ordered=km.cloud("uniform")[1]))
    idx, d2 = ops.knn(_dev(p[:0]), 3, queries=_dev(p[:5]))          # no points: every row is the pad
    assert idx.shape == (5, 3) and bool((idx == -1).all()) and bool(torch.isinf(d2).all())


@pytest.mark.parametrize("name", ["uniform", "lattice", "clusters"])
def test_shell_and_candidate_totals_equal_the_restated_search(name):
    p, ordered = km.cloud(name)
    q, q_ordered = km.cloud_queries(name)
    for k in (1, 16):
        for R in RESOLUTIONS:
            own, sep = _knn(p, k, R, return_stats=True)[2], _knn(p, k, R, q, return_stats=True)[2]
            if R == 0:
                assert (own["shells"], own["candidates"]) == (0, len(p) * len(p)) and (sep["shells"], sep["candidates"]) == (0, len(q) * len(p))
            else:
                r = km.default_resolution(len(p)) if R is None else R
                assert (own["shells"], own["candidates"]) == km.knn_grid(p, k, r, ordered=ordered)[2], (k, R)
                assert (sep["shells"], sep["candidates"]) == km.knn_grid(p, k, r, q, ordered=q_ordered)[2], (k, R)
            assert own["placed"] >= min(k, len(p) - 1) * len(p) and sep["placed"] >= min(k, len(p)) * len(q)


@functools.lru_cache(maxsize=None)
def _sensors(name):
    p, _ = km.cloud(name)
    rng = np.random.default_rng(len(name))
    d = rng.normal(size=(len(p), 3))
    ext = max(float((p.max(axis=0) - p.min(axis=0)).max()), 2.0 ** -18)
    s = p.mean(axis=0) + 3.0 * ext * d / np.linalg.norm(d, axis=1, keepdims=True)
    s.setflags(write=False)
    return s


@pytest.mark.parametrize("name", ["uniform", "lattice", "flat", "shifted_sphere"])
def test_scan_operations_equal_the_model_bit_for_bit(name):
    from dgnn_amd import ops
    p, ordered = km.cloud(name)
    for k in (6, 16):
        idx, d2 = km.knn(p, k, ordered=ordered)
        m = ops.knn_mean_distance(_dev(d2), _dev(idx)).cpu().numpy()
        assert np.array_equal(_bits(m), _bits(km.mean_distance(d2, idx)))
        want_keep, want = km.outlier_mask(p, k=k, std_ratio=1.5, ordered=ordered)
        for R in (0, None):
            keep, st = ops.outlier_mask(_dev(p), k=k, std_ratio=1.5, grid_resolution=R)
            assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), want_keep) and st["n_removed"] == want["n_removed"]
            assert np.array_equal(_bits(st["mean_distance"].cpu().numpy()), _bits(want["mean_distance"]))
            for key in ("mu", "sigma", "threshold"):
                assert _bits(st[key]) == _bits(want[key]), key
        for sensors in (None, _sensors(name)):
            want_n, want_e = km.normals(p, k=k, sensors=sensors, ordered=ordered)
            nrm, eig = ops.estimate_normals(_dev(p), k=k, sensors=_dev(sensors))
            assert np.array_equal(_bits(nrm.cpu().numpy()), _bits(want_n)) and np.array_equal(_bits(eig.cpu().numpy()), _bits(want_e))
    assert 0 < want["n_removed"] < len(p)


def test_the_scan_operations_refuse_too_few_points():
    from dgnn_amd import ops
    p = _dev(km.small(2))
    with pytest.raises(ValueError):
        ops.outlier_mask(p[:1])
    with pytest.raises(ValueError):
        ops.estimate_normals(p)
    keep, st = ops.outlier_mask(p)          # two points: one neighbour each, the same distance
    assert bool(keep.all()) and st["sigma"] == 0.0 and st["n_removed"] == 0
    with pytest.raises(ValueError, match="neighbour index"):
        from dgnn_amd._lib import lib, ptr, stream_ptr
        q = _dev(km.small(4))
        bad = torch.tensor([[1], [2], [4], [0]], dtype=torch.int32, device=DEV)
        out = torch.empty(4, 3, dtype=torch.float64, device=DEV)
        ops._check_value(lib().dgnn_knn_normals(ptr(q), 4, ptr(bad), 1, None, ptr(out), ptr(torch.empty_like(out)), ptr(torch.empty(256, dtype=torch.uint8, device=DEV)),
                                                stream_ptr()), "dgnn_knn_normals")
