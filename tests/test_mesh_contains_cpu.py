"""The CPU side of the mesh occupancy query (no device):
* tests/mesh_contains_model.py (all pairs, fp64) == tests/golden/mesh_contains.npz, the reference's own MeshIntersector on three meshes
  (tests/golden/make_golden_contains.py), exactly;
* the model's answer does not depend on the candidate grid: the lists of a grid at R and of coarser ones give the all-pairs answer;
* sample_mesh.read_off on both header forms; a points.npz written by sample_mesh's writer read back by generate_mesh's loader.
"""
import os

import numpy as np
import pytest

import mesh_contains_model as mc
from helpers import gold

MESHES = ["tet", "cube", "sphere"]


@pytest.mark.parametrize("name", MESHES)
def test_model_equals_the_reference_fixture(name):
    g = gold("mesh_contains.npz")
    v, f = {"tet": mc.tetrahedron, "cube": mc.cube, "sphere": mc.sphere_interface}[name]()
    assert np.array_equal(v, g[name + "_vertices"]) and np.array_equal(f, g[name + "_faces"])     # the fixture's meshes are the model's
    got, n_disagree = mc.contains(v, f, g[name + "_points"])
    assert np.array_equal(got, g[name + "_contains"])
    assert n_disagree == 0 and 0 < got.sum() < len(got)


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("R", [512, 8])
def test_model_does_not_depend_on_the_binning(name, R):
    v, f = {"tet": mc.tetrahedron, "cube": mc.cube, "sphere": mc.sphere_interface}[name]()
    pts = mc.adversarial_points(v, f, 600, seed=5)
    want = mc.contains(v, f, pts, R)
    sizes = []
    for shift in (0, 2, 10):
        pairs = mc.candidates(v, f, pts, R, shift)
        sizes.append(len(pairs[0]))
        got = mc.contains_from_candidates(v, f, pts, pairs, R)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], (name, R, shift)
    assert sizes[0] <= sizes[1] <= sizes[2]                      # coarser grids only add candidates
    p = mc.rescale(pts, *mc.frame(v, f, R))
    with np.errstate(invalid="ignore"):
        n_in = int(((0 <= p).all(axis=1) & (p[:, :2] < R).all(axis=1) & (p[:, 2] <= R)).sum())
    assert sizes[2] == n_in * len(f)                             # one cell: every triangle for every point in the box


def test_cube_lattice_ties_and_the_open_cube():
    """The lattice through the cube meets every tie of the definition (0 < u, sum_uv < abs_detA, depth >= z * abs_n_2).  None of them
    makes the two parities differ on a CLOSED cube: its side faces project to segments (detA == 0), a point strictly inside a projected
    triangle meets one top and one bottom triangle, the top one is above (depth >= z everywhere in the box), the bottom one below, or
    above as well at z == min, and a point on the faces' diagonal x == y meets none.  The parities differ once the top is taken away."""
    g = gold("mesh_contains.npz")
    v, f = mc.cube()
    lat = mc.lattice(-1, 6)
    got, n_disagree = mc.contains(v, f, lat)
    assert np.array_equal(got, g["cube_lattice_contains"]) and n_disagree == 0
    x, y, z = lat.T
    assert np.array_equal(got, (0 < x) & (x < 4) & (0 < y) & (y < 4) & (x != y) & (0 < z) & (z <= 4))       # the ties, as argued above
    got, n_disagree = mc.contains(v, f[:-2], g["cube_points"])
    assert np.array_equal(got, g["cube_open_contains"]) and not got.any()
    assert n_disagree >= int(g["cube_contains"].sum()) > 0          # under the missing top: one crossing below, none above


OFF_BODY = """8 12 0
0 0 0
0 0 1
0 1 0
0 1 1  # a comment
1 0 0
1 0 1
1 1 0
1 1 1

3 0 1 3
3 0 3 2
3 4 6 7
3 4 7 5
3 0 4 5
3 0 5 1
3 2 3 7
3 2 7 6
3 0 2 6
3 0 6 4
3 1 5 7
3 1 7 3
"""


@pytest.mark.parametrize("header", ["OFF\n", "OFF", "# made by hand\nOFF\n"])
def test_read_off_header_forms(tmp_path, header):
    from dgnn_amd.processing.sample_mesh import read_off
    path = os.path.join(str(tmp_path), "cube.off")
    with open(path, "w") as fh:
        fh.write(header + OFF_BODY)
    v, f = read_off(path)
    cv, cf = mc.cube(0.0, 1.0)
    assert v.dtype == np.float64 and f.dtype == np.int32
    assert np.array_equal(v, cv) and np.array_equal(f, cf)


def test_read_off_refuses_other_files(tmp_path):
    from dgnn_amd.processing.sample_mesh import read_off
    path = os.path.join(str(tmp_path), "quad.off")
    with open(path, "w") as fh:
        fh.write("OFF\n4 1 0\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    with pytest.raises(ValueError, match="only triangles"):
        read_off(path)
    with open(path, "w") as fh:
        fh.write("ply\n")
    with pytest.raises(ValueError, match="not an OFF"):
        read_off(path)


@pytest.mark.parametrize("float16", [False, True])
@pytest.mark.parametrize("n", [1, 8, 1003])
def test_points_file_round_trip(tmp_path, float16, n):
    from dgnn_amd.processing.generate_mesh import _occupancy_file, load_occupancy
    from dgnn_amd.processing.sample_mesh import write_points_file
    from dgnn_amd.config import Config
    rng = np.random.default_rng(n)
    pts = rng.random((n, 3)) - 0.5
    occ = rng.random(n) < 0.4
    data = Config(path=str(tmp_path), id="m", category="", filename="0")
    os.makedirs(os.path.join(str(tmp_path), "eval", "m"))
    write_points_file(_occupancy_file(data), pts, occ, float16=float16)
    raw = np.load(_occupancy_file(data))
    assert set(raw.files) == {"points", "occupancies", "loc", "scale"} and raw["occupancies"].dtype == np.uint8
    assert len(raw["occupancies"]) == (n + 7) // 8 and np.array_equal(raw["loc"], np.zeros(3)) and float(raw["scale"]) == 75.0
    got_pts, got_occ = load_occupancy(_occupancy_file(data))
    assert got_pts.dtype == (np.float16 if float16 else np.float32) and np.array_equal(got_pts, pts.astype(got_pts.dtype))
    assert np.array_equal(got_occ.astype(bool), occ) and len(got_occ) == n
