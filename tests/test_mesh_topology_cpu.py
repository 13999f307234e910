"""The CPU model of the exported mesh (tests/mesh_topology_model.py) on cases with known answers."""
import numpy as np
import pytest

import mesh_metrics_model as mm
import mesh_topology_model as mt

# two tetrahedra on the points below: 0 1 2 3 is positively oriented; 4 5 6 shift it
PTS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 2, 2], [3, 2, 2], [2, 3, 2], [2, 2, 3]], dtype=np.float64)


def test_one_tetrahedron_is_closed_and_outward():
    faces = np.array(mt.tetra_faces((0, 1, 2, 3)))
    top = mt.topology(faces)
    assert top == dict(n_edges=6, boundary_edges=0, nonmanifold_edges=0, nonmanifold_vertices=0, winding_mismatch_edges=0, watertight=1)
    assert abs(mt.signed_volume(PTS[:4], faces) - 1.0 / 6.0) < 1e-15
    # the orientation rule on the scene of one cell: every hull facet wound away from it
    scene = mm.scene_from_points(PTS[:4])
    faces, und = mt.orient_interface(scene, np.zeros(1, np.int32), np.arange(4, dtype=np.int32))
    assert und == 0 and abs(mt.signed_volume(PTS[:4], faces) - 1.0 / 6.0) < 1e-15


def test_two_tetrahedra_sharing_a_vertex():
    faces = np.array(mt.tetra_faces((0, 1, 2, 3)) + mt.tetra_faces((3, 5, 6, 7)))
    top = mt.topology(faces)
    assert top["nonmanifold_vertices"] == 1 and top["nonmanifold_edges"] == 0 and top["boundary_edges"] == 0
    assert top["n_edges"] == 12 and top["watertight"] == 0


def test_two_tetrahedra_sharing_an_edge():
    faces = np.array(mt.tetra_faces((0, 1, 2, 3)) + mt.tetra_faces((0, 1, 6, 7)))
    top = mt.topology(faces)
    assert top["nonmanifold_edges"] == 1 and top["nonmanifold_vertices"] == 0     # Open3D: the fan at 0 and 1 is connected through (0, 1)
    assert top["n_edges"] == 11 and top["winding_mismatch_edges"] == 0 and top["watertight"] == 0


def test_exact_sign_where_fp64_fails():
    scene = mt.regular_grid_scene()
    t = scene["tetrahedra"].astype(np.int64)
    p = [scene["vertices"][t[:, k]] for k in range(4)]
    exact = mt.orient_sign(*p)
    assert (exact != mt.naive_sign(*p)).any()
    for i in np.nonzero(exact != mt.naive_sign(*p))[0][:5]:
        d = mt.exact_det(*(q[i] for q in p))
        assert exact[i] == (d > 0) - (d < 0)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("labelling", ["sphere", "random"])
def test_oriented_interface_is_consistent_and_encloses_the_inside_cells(seed, labelling):
    scene = mm.random_scene(3000, seed=seed)
    n = len(scene["tetrahedra"])
    labels = mm.sphere_labels(scene) if labelling == "sphere" else (np.random.default_rng(seed).random(n) > 0.1).astype(np.int32)
    ids = mm.interface_ids(labels, scene["nfacets"])
    faces, und = mt.orient_interface(scene, labels, ids)
    assert und == 0
    assert mt.topology(faces)["winding_mismatch_edges"] == 0
    want = mt.inside_volume(scene, labels)
    assert abs(mt.signed_volume(scene["vertices"], faces) - want) <= 1e-9 * want
    faces_c, kept = mt.compact(faces)
    assert np.array_equal(kept[faces_c], faces) and (np.diff(kept) > 0).all()
    assert np.array_equal(np.unique(faces_c), np.arange(len(kept)))
