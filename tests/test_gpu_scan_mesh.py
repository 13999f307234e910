"""processing.scan_mesh against the composition in tests/ray_cast_model.py: points, normals, sensors and stats exactly before
the noise, the noise within the bound the jitter_points tests use, and the chain scan -> triangulation -> build_scene_features."""
import functools

import numpy as np
import pytest
import torch

import mesh_contains_model as mc
import ray_cast_model as rc
import scene_features_model as sf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return mc.cube(0.2, 0.8) if name == "cube" else mc.sphere_interface(300)


def _aims(mesh, n, seed):
    """the device's surface samples of scan_mesh's first step (their cumulative areas are the device's own)"""
    from dgnn_amd import ops
    pts, face = ops.sample_interface(torch.from_numpy(mesh[0]).to(DEV), torch.from_numpy(mesh[1]).to(DEV), None, n, seed=rc.sub_seeds(seed)[0])
    return pts.cpu().numpy(), face.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _want(name, n, cameras, seed, noise=0.0, outliers=0.0):
    mesh = _mesh(name)
    aims, aim_face = _aims(mesh, n, seed)
    return rc.scan_mesh(*mesh, aims, aim_face, rc.camera_positions(*mesh, cameras, 2.0, seed), noise, outliers, seed)


def _ulp32(a, b):          # the bound of test_generators_match_the_model (tests/test_gpu_mesh_contains.py)
    a, b = a.astype(np.float32), b.astype(np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.maximum(np.spacing(np.abs(a)), np.spacing(np.abs(b))).astype(np.float64)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name,n,cameras,seed", [("cube", 3000, 10, 0), ("sphere", 3000, 10, 0), ("sphere", 777, 3, 2 ** 40 + 5)])
def test_a_scan_equals_the_model(name, n, cameras, seed):
    from dgnn_amd.processing.scan_mesh import SCAN_STATS, scan_mesh
    mesh = _mesh(name)
    got = scan_mesh(*mesh, points=n, cameras=cameras, seed=seed, device=DEV)
    want = _want(name, n, cameras, seed)
    print("%s: stats %s (model %s)" % (name, got["stats"], want["stats"]))
    assert got["stats"] == want["stats"] and list(got["stats"]) == list(SCAN_STATS) and got["stats"]["misses"] <= 0.01 * n
    for key in ("points", "normals", "gt_normals", "sensor_position"):
        assert got[key].dtype == np.float64 and np.array_equal(_bits(got[key]), _bits(want[key])), key
    assert np.array_equal(got["cameras"], rc.camera_positions(*mesh, cameras, 2.0, seed))
    # noise = 0, outliers = 0: one point per hit, every normal towards its sensor, the hit (not the aim) is the point
    hits = got["stats"]["hits"]
    assert len(got["points"]) == hits == len(got["hit_face"]) and (got["hit_face"] >= 0).all()
    assert (rc._dot(got["normals"], got["sensor_position"] - got["points"]) >= 0).all()
    assert got["stats"]["other_face"] > 0.3 * n          # the aims on the far side gave the near side


def test_noise_and_outliers():
    from dgnn_amd.processing.scan_mesh import scan_mesh
    mesh = _mesh("sphere")
    plain = _want("sphere", 3000, 10, 0)
    hits = plain["stats"]["hits"]
    got = scan_mesh(*mesh, points=3000, cameras=10, noise=0.005, outliers=0.33, seed=0, device=DEV)
    want = _want("sphere", 3000, 10, 0, 0.005, 0.33)
    n_out = int(round(0.33 * hits))
    assert got["stats"] == plain["stats"] and len(got["points"]) == hits + n_out == len(want["points"])
    assert _ulp32(got["points"][:hits], want["points"][:hits]).all() and not np.array_equal(got["points"][:hits], plain["points"])
    for key in ("normals", "gt_normals", "sensor_position"):          # the noise moves the points only; the outliers are exact
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key
    assert np.array_equal(_bits(got["points"][hits:]), _bits(want["points"][hits:]))
    assert (got["gt_normals"][hits:] == 0).all() and (got["hit_face"][hits:] == -1).all() and (got["hit_face"][:hits] >= 0).all()
    assert np.allclose(np.linalg.norm(got["normals"][hits:], axis=1), 1.0, rtol=1e-14)
    only_out = scan_mesh(*mesh, points=3000, cameras=10, outliers=0.33, seed=0, device=DEV)
    assert np.array_equal(_bits(only_out["points"][:hits]), _bits(plain["points"])) and len(only_out["points"]) == hits + n_out
    # the caller's sensors take the cameras' place
    sensors = np.array([[3.0, 0.5, 0.5], [0.5, -2.0, 0.5]])
    own = scan_mesh(*mesh, points=500, sensors=sensors, seed=4, device=DEV)
    aims, aim_face = _aims(mesh, 500, 4)
    want_own = rc.scan_mesh(*mesh, aims, aim_face, sensors, seed=4)
    assert np.array_equal(_bits(own["points"]), _bits(want_own["points"])) and np.array_equal(own["sensor_position"], want_own["sensor_position"])
    assert set(map(tuple, own["sensor_position"])) == set(map(tuple, sensors))


def test_export_scan_round_trips(tmp_path):
    from dgnn_amd.processing.scan_mesh import SCAN_KEYS, export_scan
    mesh = _mesh("cube")
    path = str(tmp_path / "scan" / "4.npz")
    scan = export_scan(*mesh, path, points=1000, cameras=15, noise=0.0025, outliers=0.1, seed=3, device=DEV)
    z = np.load(path)
    assert z.files == list(SCAN_KEYS) == ["points", "normals", "gt_normals", "sensor_position", "cameras", "noise", "outliers"]
    assert all(z[k].dtype == np.float64 for k in z.files)
    for k in ("points", "normals", "gt_normals", "sensor_position"):
        assert z[k].shape == (len(scan["points"]), 3) and np.array_equal(_bits(z[k]), _bits(scan[k])), k
    assert z["cameras"].shape == z["noise"].shape == z["outliers"].shape == () and (float(z["cameras"]), float(z["noise"]), float(z["outliers"])) == (15.0, 0.0025, 0.1)


def test_a_scan_feeds_the_scene_features():
    """mesh -> scan_mesh -> scipy's Delaunay in the triangulator's place -> build_scene_features: every scan point is a vertex and casts
    (or shares) a ray"""
    from scipy.spatial import Delaunay

    from dgnn_amd.processing.scan_mesh import scan_mesh
    from dgnn_amd.processing.scene_features import build_scene_features
    scan = scan_mesh(*_mesh("sphere"), points=1500, cameras=10, seed=1, device=DEV)
    pts = np.unique(scan["points"], axis=0)
    tets = Delaunay(pts).simplices.astype(np.int32)
    assert len(np.unique(tets)) == len(pts)
    facets, nfacets = sf.facets_from_tets(tets)
    out = build_scene_features(dict(vertices=pts, tetrahedra=tets, facets=facets, nfacets=nfacets), np.zeros(len(tets), dtype=np.int32), scan["points"],
                               scan["sensor_position"], device=DEV)
    st = out["stats"]
    print(st)
    assert st["unmatched_points"] == 0 and st["points"] == len(scan["points"]) == scan["stats"]["hits"]
    assert st["used"] + st["duplicates"] + st["degenerate"] == len(scan["points"]) and st["used"] == len(pts) and st["degenerate"] == 0
