"""ops.point_mesh_distance (dgnn_point_mesh_distance) against the all-pairs numpy model tests/mesh_distance_model.py: d2, face,
closest point and region bit for bit, whatever the grid resolution, and again on a rerun."""
import functools

import numpy as np
import pytest
import torch

import mesh_contains_model as mc
import mesh_distance_model as md

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RESOLUTIONS = (0, 1, 2, 7, 64, None)


def _integer_cube():
    return mc.cube(0.0, 4.0)


def _nan_neighbour():
    return np.array([[np.nan, 1.0, 2.0], [0.25, 0.5, 0.125], [1.5, 0.75, 0.25], [0.5, 1.75, 1.0]]), np.array([[1, 2, 3]], dtype=np.int32)


def _shifted_sphere():
    v, f = mc.sphere_interface(300)
    return 2.0 ** 20 + v * 2.0 ** -20, f


MESHES = {
    "cube": lambda: mc.cube(0.2, 0.8),
    "integer_cube": _integer_cube,
    "tetrahedron": mc.tetrahedron,
    "nan_neighbour": _nan_neighbour,
    "sphere": lambda: mc.sphere_interface(300),
    "shifted_sphere": _shifted_sphere,
    "flat": md.flat_mesh,
    "degenerate": md.degenerate_mesh,
    "unequal": lambda: md.unequal_mesh(500),
    "sphere_larger": lambda: mc.sphere_interface(900, seed=3),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """the mesh, about 2000 query points and the model's answer, computed once"""
    v, f = MESHES[name]()
    q = md.query_points(v, f, 1500, seed=len(name))
    want = md.distance(v, f, q)
    for a in (v, f, q) + want:
        a.setflags(write=False)
    return v, f, q, want


def _run(v, f, q, R, **kw):
    from dgnn_amd import ops
    out = ops.point_mesh_distance(torch.from_numpy(np.array(v)).to(DEV), torch.from_numpy(np.array(f)).to(DEV), torch.from_numpy(np.array(q)).to(DEV),
                                  grid_resolution=R, **kw)
    return tuple(o.cpu().numpy() if isinstance(o, torch.Tensor) else o for o in out)


def _assert_equal_bits(got, want):
    d2, face, closest, region = got[:4]
    assert d2.dtype == np.float64 and face.dtype == np.int32 and closest.dtype == np.float64 and region.dtype == np.uint8
    assert np.array_equal(d2.view(np.int64), want[0].view(np.int64))
    assert np.array_equal(face, want[1])
    assert np.array_equal(closest.view(np.int64), want[2].view(np.int64))
    assert np.array_equal(region, want[3])


@pytest.mark.parametrize("name", sorted(MESHES))
def test_every_resolution_equals_the_model_bit_for_bit(name):
    v, f, q, want = _case(name)
    assert 1500 <= len(q) <= 2800
    assert len(np.unique(want[3])) == 7          # every region occurs
    from dgnn_amd import ops
    first = None
    for R in RESOLUTIONS:
        got = _run(v, f, q, R, return_d2=True, return_stats=True)
        _assert_equal_bits(got, want)
        if R == 0:
            assert got[4]["faces_evaluated"] == len(q) * len(f) and got[4]["entries"] == 0
            first = got
        else:
            assert got[4]["entries"] >= len(f) and 1 <= got[4]["max_shells"] <= (R or ops.default_grid_resolution(len(f)))
    again = _run(v, f, q, None, return_d2=True)
    _assert_equal_bits(again, first)                                    # a rerun, and the default against no grid, in every byte
    dist = _run(v, f, q, None)[0]
    assert np.array_equal(dist, np.sqrt(want[0]))                        # sqrt is correctly rounded on both sides


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_point_counts(n):
    v, f, q, want = _case("sphere")
    for R in (0, None):
        got = _run(v, f, q[:n], R, return_d2=True)
        assert got[0].shape == (n,) and got[2].shape == (n, 3)
        _assert_equal_bits(got, tuple(w[:n] for w in want))


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_narrow_points_are_promoted_exactly(dtype):
    v, f, q, _ = _case("cube")
    qn = q[:300].astype(dtype)
    qn = qn[np.isfinite(qn).all(axis=1)]
    _assert_equal_bits(_run(v, f, qn, None, return_d2=True), md.distance(v, f, qn.astype(np.float64)))


def test_refusals():
    from dgnn_amd._lib import DgnnError
    v, f, q, _ = _case("cube")
    with pytest.raises(ValueError, match="without faces"):
        _run(v, np.zeros((0, 3), np.int32), q[:4], None)
    bad = f.copy()
    bad[3, 1] = len(v)
    for R in (0, 4):
        with pytest.raises(ValueError, match="out of range"):
            _run(v, bad, q[:4], R)
        vv = v.copy()
        vv[int(f[0, 0]), 1] = np.inf
        with pytest.raises(ValueError, match="non-finite"):
            _run(vv, f, q[:4], R)
        qq = q[:70].copy()
        qq[69, 2] = np.nan
        with pytest.raises(ValueError, match="non-finite"):
            _run(v, f, qq, R)
    for R in (-1, 1025):
        with pytest.raises(DgnnError, match="grid_resolution"):
            _run(v, f, q[:4], R)
    with pytest.raises(ValueError):
        _run(v, f, q[:4].astype(np.int64), None)


# ---- deep shells: a mesh of 28 560 faces, queries that read tens of shells on their own ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _deep_case():
    v, f = md.uv_sphere(120, 120)
    groups = md.deep_queries()
    want = {k: md.distance(v, f, q, chunk=16) for k, q in groups.items()}
    return v, f, groups, want


@pytest.mark.parametrize("group", ["near", "inside", "outside", "around"])
def test_deep_shells_equal_the_model_bit_for_bit(group):
    from dgnn_amd import ops
    v, f, groups, want = _deep_case()
    q, R0 = groups[group], ops.default_grid_resolution(len(f))
    assert len(f) == 28560 and R0 == 84
    for R in (0, 60, None):
        got = _run(v, f, q, R, return_d2=True, return_stats=True)
        _assert_equal_bits(got, want[group])
        st = got[4]
        print(group, R, st)
        if R == 0:
            continue
        if group == "near":
            assert st["max_shells"] <= 3
        elif group == "inside":          # the centre is at the same distance from every vertex: it reads the whole grid, shell by shell
            assert st["max_shells"] >= (R or R0) // 2 and st["shells"] > 3 * len(q)
        elif group == "outside":
            # p = 200 (1, 1, 1): best d2 = (200 sqrt(3) - 1)^2 = 119 308; after s shells of width h = 2 / R the bound is (199 + s h)^2 + 2 * 199^2,
            # above d2 once s h > 1.27, i.e. after 0.64 R shells: more than half the grid, and well short of all of it.  A query 200 away on one
            # axis reads its two other axes out (R / 2 shells and a few) and is then stopped by the one side left.
            assert (R or R0) // 2 <= st["max_shells"] < (R or R0)
        # ("around": a few extents away the box terms are too small to stop every query before the grid ends: bit for bit only)


def test_deep_shells_stats_equal_the_restated_search():
    """the shells read and the faces evaluated, query by query what tests/mesh_distance_model.distance_grid counts: the shell enumeration, the
    skip rule and the stopping bound with its box terms, none of which the answer alone can show"""
    v, f, groups, want = _deep_case()
    q = np.concatenate([groups["outside"][:12], groups["inside"][1:4], groups["near"][:5]])
    model = md.distance_grid(v, f, q, 60)
    got = _run(v, f, q, 60, return_d2=True, return_stats=True)
    _assert_equal_bits(got, model[:4])
    assert (got[4]["max_shells"], got[4]["shells"], got[4]["faces_evaluated"]) == model[4]
    assert model[4][0] >= 30
