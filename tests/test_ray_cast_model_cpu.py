"""tests/ray_cast_model.py on its own (no GPU): the first-hit rule on configurations whose answer is known by hand, the exact signs at
shared edges and vertices, the scanner's host pieces against dgnn_amd.processing.scan_mesh, and the miss share of the scanner's own rays."""
import functools

import numpy as np
import pytest

import mesh_contains_model as mc
import mesh_metrics_model as mm
import ray_cast_model as rc


def int_cube():
    return mc.cube(0.0, 4.0)


scanner_rays = rc.scanner_rays


@functools.lru_cache(maxsize=None)
def mesh(name):
    return {"cube": lambda: mc.cube(0.2, 0.8), "sphere": lambda: mc.sphere_interface(300), "tetrahedron": mc.tetrahedron}[name]()


def test_a_ray_through_the_integer_cube():
    v, f = int_cube()
    o, g = np.array([[2.25, 1.5, -4.0]]), np.array([[2.25, 1.5, 0.0]])          # straight up through z = 0 and z = 4, off every diagonal
    face, t, p, st = rc.first_hit(v, f, o, g)
    assert t[0] == 1.0 and np.array_equal(p[0], [2.25, 1.5, 0.0]) and (v[f[face[0]]][:, 2] == 0).all()
    assert st == dict(hits=1, skipped=0, degenerate=0, exact_used=0)
    far = rc.first_hit(v, f, o, g, t_min=1.5)                                    # between the two crossings
    assert far[1][0] == 2.0 and (v[f[far[0][0]]][:, 2] == 4).all()
    assert rc.first_hit(v, f, o, g, t_min=2.0)[0][0] == -1                       # t <= t_min is dropped
    away = rc.first_hit(v, f, o, 2 * o - g)
    assert away[0][0] == -1 and away[1][0] == 0 and np.array_equal(away[2][0], [0, 0, 0]) and away[3]["hits"] == 0
    same = rc.first_hit(v, f, o, o)
    assert same[0][0] == -1 and same[3] == dict(hits=0, skipped=1, degenerate=0, exact_used=0)


def test_exact_zeros_cross_every_incident_face_and_ties_go_to_the_lowest_id():
    v, f = int_cube()
    o = np.array([[9.0, 7.0, -5.0]])
    corner = np.array([[4.0, 4.0, 0.0]])
    face, t, p, st = rc.first_hit(v, f, o, corner)
    incident = np.nonzero((v[f] == corner[0]).all(axis=2).any(axis=1))[0]
    assert t[0] == 1.0 and face[0] == incident.min() and np.array_equal(p[0], corner[0]) and st["exact_used"] >= 2
    # the midpoint of the diagonal of the bottom face lies on two faces: both are crossed at t = 1
    mid = np.array([[2.0, 2.0, 0.0]])
    face, t, _, st = rc.first_hit(v, f, np.array([[2.0, 2.0, -3.0]]), mid)
    shared = np.nonzero((v[f][:, :, 2] == 0).all(axis=1))[0]
    assert len(shared) == 2 and face[0] == shared.min() and t[0] == 1.0 and st["exact_used"] >= 1
    # a line in the plane z = 0 crosses no face of that plane; along the edge y = z = 0 it crosses the faces that meet the edge's ends
    in_plane = rc.first_hit(v, f, np.array([[-1.0, 1.0, 0.0]]), np.array([[0.0, 1.5, 0.0]]))
    assert in_plane[0][0] >= 0 and not (v[f[in_plane[0][0]]][:, 2] == 0).all()
    along = rc.first_hit(v, f, np.array([[-2.0, 0.0, 0.0]]), np.array([[-1.0, 0.0, 0.0]]))
    assert along[0][0] >= 0 and along[1][0] == 2.0 and not ((v[f[along[0][0]]][:, 1] == 0).all() or (v[f[along[0][0]]][:, 2] == 0).all())


def test_degenerate_faces_are_never_hit_and_a_cancelling_denominator_is_counted():
    v, f = int_cube()
    f2 = np.concatenate([[[0, 0, 7], [0, 7, 7]], f, [[0, 3, 3]]]).astype(np.int32)          # repeated ids before and after the cube
    v2 = np.concatenate([v, [[2.0, 2.0, 2.0], [1.0, 1.0, 1.0], [3.0, 3.0, 3.0]]])
    f2 = np.concatenate([f2, [[8, 9, 10]]]).astype(np.int32)                                # three points on one line: no area
    o, g = np.array([[2.25, 1.5, -4.0], [9.0, 9.0, 9.0]]), np.array([[2.25, 1.5, 0.0], [0.0, 0.0, 0.0]])
    want = rc.first_hit(v, f, o, g)
    got = rc.first_hit(v2, f2, o, g)
    assert np.array_equal(got[0], want[0] + 2) and np.array_equal(got[1], want[1]) and got[3]["degenerate"] == 0
    # n = (3, 0, -1), d = (fl(1/3), 0, 1): the line crosses the face at the origin, and 3 fl(1/3) rounds to 1, so n . d is 0 in fp64
    x = 1.0 / 3.0
    tv = np.array([[-0.25, -0.25, -0.75], [-0.25, 0.75, -0.75], [0.75, -0.25, 2.25]])
    res = rc.first_hit(tv, np.array([[0, 1, 2]], dtype=np.int32), np.zeros((1, 3)), np.array([[x, 0.0, 1.0]]))
    assert res[0][0] == -1 and res[3] == dict(hits=0, skipped=0, degenerate=1, exact_used=0)


@pytest.mark.parametrize("name", ["cube", "sphere", "tetrahedron"])
def test_scanner_rays_miss_share_and_the_filter_only_rule(name):
    """4096 rays of the scanner (10 cameras at distance 2, seed 0): at most 1 % may miss the closed mesh they aim at, and away from exact
    zeros the fp64 rule alone gives the same answer"""
    v, f = mesh(name)
    o, g, aim_face, cams = scanner_rays(v, f)
    face, t, p, st = rc.first_hit(v, f, o, g)
    misses = int((face < 0).sum())
    print("%s: %d faces, %d misses of %d, %d hits on another face, exact stage %d" % (name, len(f), misses, len(o), int((face != aim_face).sum()), st["exact_used"]))
    assert misses <= 0.01 * len(o) and st["skipped"] == 0 and st["degenerate"] == 0 and st["hits"] == len(o) - misses
    hit = face >= 0
    # the aim is on the surface up to its fp32 rounding (5e-8 here): nothing is hit behind it, but for a grazing ray
    assert (t[hit] > 0).all() and (t[hit] <= 1 + 1e-3).all() and (t[hit] <= 1 + 1e-6).mean() > 0.99
    lite_face, lite_t = rc.filter_only_first_hit(v, f, o, g)
    assert (lite_face != face).sum() <= 4 and np.array_equal(lite_t[lite_face == face], t[lite_face == face])


def test_the_scanner_host_pieces_equal_the_package():
    from dgnn_amd import ops
    from dgnn_amd.processing import scan_mesh as sm
    v, f = mesh("sphere")
    for n, dist, seed in ((10, 2.0, 0), (1, 1.5, 7), (50, 3.0, 2 ** 40 + 3)):
        got, want = sm.camera_positions(v, f, n, dist, seed), rc.camera_positions(v, f, n, dist, seed)
        assert got.dtype == np.float64 and got.shape == (n, 3) and np.array_equal(got, want)
        centre, radius = rc.frame(v, f)
        assert np.allclose(np.linalg.norm(got - centre, axis=1), dist * radius, rtol=1e-14)
    assert np.array_equal(sm.mm_hash(5, np.arange(9)), mm.mm_hash(5, np.arange(9))) and sm.SCAN_KEYS == rc.SCAN_KEYS and sm.SCAN_STATS == rc.SCAN_STATS
    unused = np.concatenate([v, [[50.0, 50.0, 50.0]]])                          # an unreferenced vertex moves nothing
    assert np.array_equal(sm.camera_positions(unused, f, 10), sm.camera_positions(v, f, 10))
    z = (sm.camera_positions(v, f, 4000, seed=1) - rc.frame(v, f)[0])[:, 2] / (2.0 * rc.frame(v, f)[1])
    assert abs(z.mean()) < 0.05 and abs((z < 0.5).mean() - 0.75) < 0.03          # uniform by area: z is uniform on [-1, 1]
    assert ops.RAY_HIT_STATS == rc.HIT_STATS
    assert [ops.default_grid_resolution(n) for n in (1, 12, 144, 10 ** 4, 10 ** 6, 10 ** 8)] == [1, 2, 6, 50, 256, 256]


def test_scan_composition_in_the_model():
    v, f = mesh("cube")
    o, g, aim_face, cams = scanner_rays(v, f, n=600)
    plain = rc.scan_mesh(v, f, g.astype(np.float32), aim_face, cams)
    st = plain["stats"]
    assert st["rays"] == 600 and st["hits"] + st["misses"] == 600 and len(plain["points"]) == st["hits"]
    assert 200 < st["other_face"] < 500          # an aim on the far side yields the near side: about half of the surface faces away from a camera
    assert (rc._dot(plain["normals"], plain["sensor_position"] - plain["points"]) >= 0).all()
    assert np.array_equal(np.abs(plain["normals"]), np.abs(plain["gt_normals"]))
    noisy = rc.scan_mesh(v, f, g.astype(np.float32), aim_face, cams, noise=0.01, outliers=0.33)
    n_out = int(round(0.33 * st["hits"]))
    assert len(noisy["points"]) == st["hits"] + n_out and (noisy["gt_normals"][st["hits"]:] == 0).all()
    assert np.allclose(np.linalg.norm(noisy["normals"][st["hits"]:], axis=1), 1.0, rtol=1e-14)
    centre, radius = rc.frame(v, f)
    assert (np.abs(noisy["points"][st["hits"]:] - centre) <= radius).all()
    d = noisy["points"][:st["hits"]] - plain["points"]
    assert 0.008 < d.std() < 0.012
