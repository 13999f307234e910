"""The CPU model of the mesh metrics (tests/mesh_metrics_model.py) against independent definitions: ray parity against the interface
triangles (the reference's check_mesh_contains) agrees with "label of Delaunay.find_simplex"; the sampler restatement; the chamfer
restatement against brute force."""
import numpy as np

import mesh_metrics_model as mm


def test_ray_parity_agrees_with_find_simplex_labels():
    for seed, n_points in ((0, 60), (1, 200), (2, 400)):
        rng = np.random.default_rng(seed)
        pts = rng.random((n_points, 3))
        scene = mm.scene_from_points(pts)
        labels = mm.sphere_labels(scene, radius=0.35)
        tris = scene["facets"][mm.interface_ids(labels, scene["nfacets"])]
        q = (rng.random((600, 3)) * 1.1 - 0.05).astype(np.float32)       # a box padded by 5 %: points outside the hull too
        inside, clean = mm.ray_parity_inside(scene["vertices"], tris, q)
        want = mm.find_simplex_occupancy(q, pts, labels)
        assert clean.mean() > 0.95 and (~want).any() and want.any()
        assert np.array_equal(inside[clean], want[clean])


def test_orientation_rule_matches_find_simplex():
    rng = np.random.default_rng(3)
    pts = rng.random((300, 3))
    scene = mm.scene_from_points(pts)
    from scipy.spatial import Delaunay
    q = rng.random((500, 3)).astype(np.float32)
    s = Delaunay(pts).find_simplex(q.astype(np.float64))
    assert (s >= 0).mean() > 0.8
    assert mm.cell_signs(scene, s[s >= 0], q[s >= 0]).all()


def test_scene_layout():
    scene = mm.random_scene(200, seed=4)
    t, f, nf = scene["tetrahedra"], scene["facets"], scene["nfacets"]
    # 4 faces per cell: interior facets counted twice, hull facets once
    assert 4 * len(t) == 2 * (nf[:, 1] >= 0).sum() + (nf[:, 1] < 0).sum()
    for i in range(0, len(f), 17):
        for c in nf[i]:
            if c >= 0:
                assert set(f[i]) <= set(t[c])


def test_hash_and_sampler_restatement():
    # splitmix64 finaliser: known values of the standard generator seeded with 0 (state advances by the golden gamma)
    got = mm.mm_hash(0, np.arange(1, 4, dtype=np.uint64))
    assert [int(x) for x in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    scene = mm.random_scene(100, seed=5)
    ids = np.arange(len(scene["facets"]), dtype=np.int32)
    areas = mm.face_areas(scene["vertices"], scene["facets"], ids)
    areas[::7] = 0.0                                                   # zero-area faces never get a sample
    cum = np.cumsum(areas)
    pts, j = mm.sample(scene["vertices"], scene["facets"], ids, cum, 20000, seed=9)
    assert (areas[j] > 0).all()
    v = scene["vertices"][scene["facets"][j]]
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    off = np.abs(np.einsum("ij,ij->i", pts - v[:, 0], n)) / np.linalg.norm(n, axis=1)
    assert off.max() < 1e-6
    a, b = mm.sample(scene["vertices"], scene["facets"], ids, cum, 50, seed=9)
    assert np.array_equal(a, pts[:50]) and np.array_equal(b, j[:50])   # a sample does not depend on how many are drawn


def test_chamfer_restatement_matches_brute_force():
    rng = np.random.default_rng(6)
    gt = rng.random((700, 3)).astype(np.float32)
    rc = (rng.random((500, 3)) * 0.9).astype(np.float32)
    d1, _ = mm.nn_brute(rc, gt)
    d2, _ = mm.nn_brute(gt, rc)
    want = 0.5 * (d1.astype(np.float64).mean() + d2.astype(np.float64).mean())
    assert abs(mm.chamfer_ckdtree(gt, rc) - want) <= 1e-6 * want
