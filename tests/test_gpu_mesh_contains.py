"""ops.mesh_contains and what is built on it (csrc/meshcontains.hip) against tests/golden/mesh_contains.npz (the reference's own
MeshIntersector) and tests/mesh_contains_model.py (all pairs, fp64).  Every occupancy comparison is exact equality of the boolean
arrays and of n_disagree: no tolerance, no excluded point."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_contains_model as mc
import mesh_metrics_model as mm
from dgnn_amd.config import Config
from helpers import gold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MESHES = ["tet", "cube", "sphere"]


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "cube_open":
        v, f = mc.cube()
        return v, f[:-2]
    return {"tet": mc.tetrahedron, "cube": mc.cube, "sphere": mc.sphere_interface}[name]()


@functools.lru_cache(maxsize=None)
def _adversarial(name):
    """about 4096 points; for the cubes also the integer lattice through them"""
    v, f = _mesh(name)
    n_fixed = len(mc.adversarial_points(v, f, 0, seed=0))
    pts = mc.adversarial_points(v, f, 4096 - n_fixed - (343 if name.startswith("cube") else 0), seed=11)
    if name.startswith("cube"):
        pts = np.concatenate([pts, mc.lattice(-1, 6)])
    return pts


@functools.lru_cache(maxsize=None)
def _want(name, R):
    v, f = _mesh(name)
    return mc.contains(v, f, _adversarial(name), R)


def _contains(v, f, p, **kw):
    from dgnn_amd import ops
    got, n_disagree = ops.mesh_contains(v, f, p, **kw)
    assert got.dtype == torch.bool and got.is_cuda and isinstance(n_disagree, int)
    return got.cpu().numpy(), n_disagree


@pytest.mark.parametrize("name", MESHES)
def test_fixture_meshes_match_the_reference(name):
    g = gold("mesh_contains.npz")
    got, n_disagree = _contains(g[name + "_vertices"], g[name + "_faces"], g[name + "_points"])
    assert np.array_equal(got, g[name + "_contains"]) and n_disagree == 0
    if name == "cube":
        v, f = _mesh("cube")
        assert np.array_equal(_contains(v, f, mc.lattice(-1, 6))[0], g["cube_lattice_contains"])
        assert np.array_equal(_contains(v, f[:-2], g["cube_points"])[0], g["cube_open_contains"])


@pytest.mark.parametrize("R", [512, 8])
@pytest.mark.parametrize("name", MESHES + ["cube_open"])
def test_adversarial_points_match_the_model(name, R):
    """uniform points in the padded box, every vertex / edge midpoint / face centroid, the box corners, points just outside each side,
    NaN and +-inf rows, the lattice through the cube; at R = 512 and R = 8 (another rescale, so another expected array).  The closed
    cube's lattice ties leave the two parities equal (tests/test_mesh_contains_cpu.py says why); on cube_open they differ under the whole
    missing top."""
    v, f = _mesh(name)
    want, want_dis = _want(name, R)
    got, n_disagree = _contains(v, f, _adversarial(name), hash_resolution=R)
    print("%s R=%d: %d points, %d inside, n_disagree %d (model %d), %d mismatches" % (name, R, len(got), got.sum(), n_disagree, want_dis, (got != want).sum()))
    assert np.array_equal(got, want) and n_disagree == want_dis
    assert 0 < want.sum() < len(want) or name == "cube_open"
    assert (want_dis > 0) == (name != "cube")          # vertices and edge points of the other meshes split the parities too
    again, again_dis = _contains(v, f, _adversarial(name), hash_resolution=R)
    assert np.array_equal(again, got) and again_dis == n_disagree


def test_the_two_resolutions_differ():
    assert not np.array_equal(_want("sphere", 512)[0], _want("sphere", 8)[0])


@pytest.mark.parametrize("name", ["cube", "sphere"])
def test_forced_coarsening_gives_the_same_answer(name):
    """max_entries below the entries of the full grid coarsens it (the plan call says by how much); the answer stays"""
    import ctypes as C
    from dgnn_amd import ops
    from dgnn_amd._lib import lib, ptr, stream_ptr
    v, f = _mesh(name)
    vt, ft = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    scratch = torch.empty(int(lib().dgnn_mesh_contains_scratch_bytes(len(v), len(f), 64)), dtype=torch.uint8, device=DEV)
    plans = []
    for cap in (2 ** 30, 1024, len(f)):
        shift, ne = C.c_int32(-1), C.c_int64(-1)
        assert lib().dgnn_mesh_contains_plan(ptr(vt), len(v), ptr(ft), len(f), 64, cap, C.byref(shift), C.byref(ne), ptr(scratch), stream_ptr()) == 0
        plans.append((shift.value, ne.value))
        assert ne.value <= cap
    assert plans[0][0] == 0 and plans[1][0] > 0 and plans[2] == (6, len(f))          # the finest that fits; one cell at the end
    full = _contains(v, f, _adversarial(name), hash_resolution=64)
    assert full[0].tolist() == mc.contains(v, f, _adversarial(name), 64)[0].tolist()
    for cap in (1024, len(f)):
        got = _contains(v, f, _adversarial(name), hash_resolution=64, max_entries=cap)
        assert np.array_equal(got[0], full[0]) and got[1] == full[1]
    with pytest.raises(Exception, match="max_entries"):
        ops.mesh_contains(v, f, _adversarial(name), hash_resolution=64, max_entries=len(f) - 1)
    assert np.array_equal(_contains(v, f, _adversarial(name), hash_resolution=64)[0], full[0])


@pytest.mark.parametrize("large_first", [True, False])
def test_one_face_over_every_cell_beside_faces_of_one_cell(large_first):
    """The entry lookup of the grid builder with very unequal boxes: one face spans the whole xy box, so it has R^2 entries, and 20
    small faces lie in one cell each, at hash_resolution 2, 3 and 8; the large face is the first of the list or the last.  Once with
    the default max_entries and once with one entry too few for the full grid, which coarsens it."""
    import ctypes as C
    from dgnn_amd._lib import lib, ptr, stream_ptr
    rng = np.random.default_rng(29)
    # the frame maps [0, 1] to [0.5, R - 0.5] and cells are int(coord): +- 0.02 about these crosses no boundary at R = 2, 3 or 8
    slots = np.array([0.14, 0.30, 0.43, 0.57, 0.70, 0.86])
    small = (slots[rng.integers(0, 6, (20, 1, 3))] + rng.uniform(-0.02, 0.02, (20, 3, 3))).reshape(60, 3)
    v = np.concatenate([np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0, 1.0]]), small])
    f = np.arange(63, dtype=np.int32).reshape(21, 3)
    if not large_first:
        f = np.roll(f, -1, axis=0)
    pts = mc.adversarial_points(v, f, 300, seed=5)
    vt, ft = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    for R in (2, 3, 8):
        want, want_dis = mc.contains(v, f, pts, R)
        scratch = torch.empty(int(lib().dgnn_mesh_contains_scratch_bytes(63, 21, R)), dtype=torch.uint8, device=DEV)
        for cap, coarsened in ((2 ** 30, False), (R * R + 19, True)):
            shift, ne = C.c_int32(-1), C.c_int64(-1)
            assert lib().dgnn_mesh_contains_plan(ptr(vt), 63, ptr(ft), 21, R, cap, C.byref(shift), C.byref(ne), ptr(scratch), stream_ptr()) == 0
            assert (shift.value > 0) == coarsened and (coarsened or ne.value == R * R + 20)
            got, n_disagree = _contains(v, f, pts, hash_resolution=R, max_entries=cap)
            print("R=%d max_entries=%d: shift %d, %d entries, %d mismatches" % (R, cap, shift.value, ne.value, (got != want).sum()))
            assert np.array_equal(got, want) and n_disagree == want_dis


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_input_types(dtype, as_tensor):
    v, f = _mesh("sphere")
    with np.errstate(over="ignore"):
        pts = _adversarial("sphere").astype(dtype)
    want = mc.contains(v, f, pts)                       # the model promotes the dtype's own values
    if as_tensor:
        got = _contains(torch.from_numpy(v), torch.from_numpy(f.astype(np.int64)), torch.from_numpy(pts).to(DEV))
    else:
        got = _contains(v, f, pts)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]


def test_empty_point_set():
    v, f = _mesh("tet")
    got, n_disagree = _contains(v, f, np.zeros((0, 3), dtype=np.float32))
    assert got.shape == (0,) and n_disagree == 0


def test_refusals_leave_the_device_usable():
    from dgnn_amd import ops
    v, f = _mesh("tet")
    pts = _adversarial("tet")
    want = _want("tet", 512)

    def good():
        got = _contains(v, f, pts)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]

    with pytest.raises(ValueError, match="without faces"):
        ops.mesh_contains(v, np.zeros((0, 3), dtype=np.int32), pts)
    good()
    flat = v.copy()
    flat[:, 1] = 0.25
    with pytest.raises(ValueError, match="no extent on axis 1"):
        ops.mesh_contains(flat, f, pts)
    good()
    for bad_id in (4, -1):
        bad = f.copy()
        bad[2, 1] = bad_id
        with pytest.raises(ValueError, match="out of range"):
            ops.mesh_contains(v, bad, pts)
        good()
    nonfinite = v.copy()
    nonfinite[3, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        ops.mesh_contains(nonfinite, f, pts)
    good()
    unused = np.concatenate([v, [[np.nan, 0, 0]]])          # a vertex no face references does not count
    assert np.array_equal(_contains(unused, f, pts)[0], want[0])
    with pytest.raises(ValueError, match="fp16, fp32 or fp64"):
        ops.mesh_contains(v, f, np.zeros((4, 3), dtype=np.int64))
    with pytest.raises(Exception, match="hash_resolution"):
        ops.mesh_contains(v, f, pts, hash_resolution=8192)
    with pytest.raises(ValueError, match="hash_resolution"):
        ops.mesh_contains(v, f, pts, hash_resolution=1)
    good()


def test_occupancy_iou_uses_compute_ious_counts():
    from dgnn_amd import ops
    v, f = _mesh("sphere")
    pts = _adversarial("sphere")
    gt = np.linalg.norm(np.nan_to_num(pts, posinf=9.0, neginf=-9.0) - 0.5, axis=1) < 0.3
    iou, occ, inter, union = ops.mesh_occupancy_iou(v, f, pts, gt)
    want = _want("sphere", 512)[0]
    assert np.array_equal(occ.cpu().numpy(), want) and (inter, union) == (int((want & gt).sum()), int((want | gt).sum()))
    assert iou == mm.iou(want, gt) and 0 < iou < 1


# ---- generators ------------------------------------------------------------------------------------------------------------------
def _ulp32(a, b):
    a, b = a.astype(np.float32), b.astype(np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.maximum(np.spacing(np.abs(a)), np.spacing(np.abs(b))).astype(np.float64)


@pytest.mark.parametrize("n", [1, 333, 5000])
def test_generators_match_the_model(n):
    from dgnn_amd import ops
    box = ops.box_points(n, 75.75, seed=7)
    assert box.dtype == torch.float64 and box.shape == (n, 3) and box.is_cuda
    want = mc.box_points(n, 75.75, 7)
    assert np.array_equal(box.cpu().numpy(), want) and np.abs(want).max() <= 75.75 / 2
    assert torch.equal(ops.box_points(n, 75.75, seed=7), box) and not torch.equal(ops.box_points(n, 75.75, seed=8), box)
    jit = ops.jitter_points(box, 0.05, seed=3)
    want_j = mc.jitter_points(want, 0.05, 3)
    assert jit.dtype == torch.float64 and _ulp32(jit.cpu().numpy(), want_j).all()
    assert torch.equal(ops.jitter_points(box, 0.05, seed=3), jit)
    if n == 5000:
        z = (want_j - want) / 0.05
        assert abs(z.mean()) < 0.05 and abs(z.std() - 1) < 0.05          # 15000 draws: 4 sigma of the mean is 0.033, of the std 0.023


def test_face_normals():
    from dgnn_amd import ops
    v, f = _mesh("sphere")
    v = np.concatenate([v, [[0.5, 0.5, 0.5], [0.6, 0.6, 0.6], [0.7, 0.7, 0.7]]])
    n0 = len(v) - 3
    f = np.concatenate([f, [[n0, n0 + 1, n0 + 2], [n0, n0, n0 + 1]]]).astype(np.int32)          # collinear, repeated: no area
    got = ops.face_normals(v, f)
    assert got.dtype == torch.float64 and got.shape == (len(f), 3)
    got = got.cpu().numpy()
    assert np.abs(got - mc.face_normals(v, f)).max() <= 2.0 ** -23
    assert np.array_equal(got[-2:], np.zeros((2, 3))) and np.abs(np.linalg.norm(got[:-2], axis=1) - 1).max() <= 2.0 ** -23
    assert np.array_equal(ops.face_normals(v, f).cpu().numpy(), got)
    bad = f.copy()
    bad[0, 0] = len(v)
    with pytest.raises(ValueError, match="out of range"):
        ops.face_normals(v, bad)
    assert ops.face_normals(v, f[:0]).shape == (0, 3)


# ---- the sample builder --------------------------------------------------------------------------------------------------------------
SPHERE_SEED = 44   # random_scene(300, seed): the first seeds leave an edge in four faces (the reference's is_watertight refuses those too)


def test_sample_mesh_writes_both_files(tmp_path, capsys):
    from dgnn_amd import ops
    from dgnn_amd.processing import sample_mesh as sm
    from dgnn_amd.processing.generate_mesh import chamfer_gpu, iou_gpu
    scene = mm.random_scene(300, SPHERE_SEED)
    labels = mm.sphere_labels(scene)
    v, f = mc.sphere_interface(300, SPHERE_SEED)
    out_dir = os.path.join(str(tmp_path), "eval", "m")
    kw = dict(pointcloud_size=1500, points_size=3000, points_uniform_ratio=0.5, points_sigma=0.05, points_padding=0.25, scale=1.0, seed=5)
    v0 = v - 0.5                                                           # the box is about the origin
    paths = sm.sample_mesh(v0, f, out_dir, **kw)
    assert paths == {"pointcloud": os.path.join(out_dir, "pointcloud.npz"), "points": os.path.join(out_dir, "points.npz")}
    pc, po = np.load(paths["pointcloud"]), np.load(paths["points"])
    assert set(pc.files) == {"points", "normals", "loc", "scale"} and set(po.files) == {"points", "occupancies", "loc", "scale"}
    assert pc["points"].dtype == np.float32 and pc["normals"].dtype == np.float32 and pc["points"].shape == pc["normals"].shape == (1500, 3)
    assert po["points"].dtype == np.float32 and po["points"].shape == (3000, 3) and po["occupancies"].dtype == np.uint8 and len(po["occupancies"]) == 375
    # the point cloud: the library's sampler and the normals of the sampled faces
    pts, face = ops.sample_interface(v0, f, None, 1500, seed=5)
    assert np.array_equal(pc["points"], pts.cpu().numpy())
    assert np.abs(pc["normals"] - mc.face_normals(v0, f)[face.cpu().numpy()]).max() <= 2.0 ** -23
    # the occupancies: mesh_contains on the fp64 points before the cast; 1500 box points by the model's formula first
    p64 = sm.sample_points(v0, f, 3000, 0.5, 0.05, 0.25, 1.0, seed=5)
    assert p64.dtype == torch.float64 and np.array_equal(p64[:1500].cpu().numpy(), mc.box_points(1500, 1.25, 6))
    assert np.array_equal(po["points"], p64.cpu().numpy().astype(np.float32))
    want, _ = mc.contains(v0, f, p64.cpu().numpy())
    occ = np.unpackbits(po["occupancies"])[:3000].astype(bool)
    assert np.array_equal(occ, want) and np.array_equal(occ, ops.mesh_contains(v0, f, p64)[0].cpu().numpy()) and 0 < occ.sum() < 3000
    # reproducible per seed; fp16 on request
    again = sm.sample_mesh(v0, f, os.path.join(str(tmp_path), "again"), float16=True, **kw)
    po2 = np.load(again["points"])
    assert po2["points"].dtype == np.float16 and np.array_equal(po2["occupancies"], po["occupancies"])
    assert np.array_equal(po2["points"], p64.cpu().numpy().astype(np.float16))
    # both files load through the metrics of generate
    shifted = dict(scene, vertices=scene["vertices"] - 0.5)
    data = Config(path=str(tmp_path), id="m", category="", filename="0")
    cells = ops.locate_points(shifted["vertices"], shifted["tetrahedra"], shifted["facets"], shifted["nfacets"], po["points"]).cpu().numpy()
    walk = (cells >= 0) & (labels[np.maximum(cells, 0)] == 0)
    assert iou_gpu(data, shifted, torch.from_numpy(labels).to(DEV)) == mm.iou(walk, occ)
    ids = mm.interface_ids(labels, scene["nfacets"])
    ch = chamfer_gpu(data, shifted, torch.from_numpy(ids).to(DEV), Config(evaluation=Config(seed=0)))
    recon, _ = ops.sample_interface(shifted["vertices"], shifted["facets"], ids, 1500, seed=0)
    assert ch == ops.chamfer_distance(torch.from_numpy(pc["points"]).to(DEV), recon) and 0 < ch < 0.1   # 1500 points on ~1.1 units of area: neighbours ~0.03 apart
    # a mesh with a hole is refused with the reference's warning, and nothing is written
    capsys.readouterr()
    holed = sm.sample_mesh(v0, f[1:], os.path.join(str(tmp_path), "holed"), **kw)
    assert holed["points"] is None and not os.path.exists(os.path.join(str(tmp_path), "holed", "points.npz")) and holed["pointcloud"] is not None
    assert "Warning: mesh holed is not watertight!Cannot sample points." in capsys.readouterr().out


# ---- generate / evaluate ---------------------------------------------------------------------------------------------------------------
def _small_scene(tmp_path):
    """tests/golden/genmesh_f4_small.npz laid out as a scene folder; the query points are the centroids of all finite cells"""
    from dgnn_amd.processing.sample_mesh import write_points_file
    g = gold("genmesh_f4_small.npz")
    scene = {k: g[k] for k in ("vertices", "tetrahedra", "facets", "nfacets")}
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "gt"))
    os.makedirs(os.path.join(root, "eval", "m"))
    np.savez(os.path.join(root, "gt", "0_3dt.npz"), **scene)
    cen = mm.centroids(scene).astype(np.float32)
    gt = np.linalg.norm(cen - cen.mean(axis=0), axis=1) < np.median(np.linalg.norm(cen - cen.mean(axis=0), axis=1))
    write_points_file(os.path.join(root, "eval", "m", "points.npz"), cen, gt)
    rng = np.random.default_rng(2)
    np.savez(os.path.join(root, "eval", "m", "pointcloud.npz"), points=(cen.mean(axis=0) + rng.standard_normal((400, 3)) * cen.std(axis=0)).astype(np.float32))
    data = Config(path=root, gtfile="gt/0", filename="0", id="m", category="", infinite=torch.from_numpy(g["infinite"]))
    return g, scene, cen, gt, data


def _clf(metrics, occupancy=None):
    clf = Config(temp=Config(graph_cut=0, fix_orientation=0, metrics=metrics, device=DEV), evaluation=Config(solver="gpu", seed=0))
    if occupancy:
        clf.evaluation.occupancy = occupancy
    return clf


def test_generate_with_mesh_occupancy_equals_the_walk(tmp_path, capsys):
    from dgnn_amd import ops
    from dgnn_amd.processing.generate_mesh import generate
    g, scene, cen, gt, data = _small_scene(tmp_path)
    pred = torch.from_numpy(g["prediction"]).to(DEV)
    mesh_m, ev_m = generate(data, pred, _clf(["iou", "chamfer"], "mesh"))
    mesh_w, ev_w = generate(data, pred, _clf(["iou", "chamfer"]))
    assert "WARNING" not in capsys.readouterr().out
    assert np.array_equal(np.asarray(mesh_m.faces), g["faces"]) and np.array_equal(np.asarray(mesh_w.faces), g["faces"])
    labels = g["prediction"][g["infinite"] == 0].argmax(axis=1).astype(np.int32)
    # per point: the model (CPU), the device query and the walk all say the same at every centroid
    want, want_dis = mc.contains(scene["vertices"], g["faces"], cen)
    assert np.array_equal(want, labels == 0) and want_dis == 0
    got, n_disagree = ops.mesh_contains(scene["vertices"], g["faces"], cen)
    _, walk, _, _ = ops.mesh_iou(scene["vertices"], scene["tetrahedra"], scene["facets"], scene["nfacets"], torch.from_numpy(labels).to(DEV), cen, gt)
    assert np.array_equal(got.cpu().numpy(), want) and n_disagree == 0 and np.array_equal(walk.cpu().numpy().astype(bool), want)
    assert ev_m["iou"] == ev_w["iou"] == mm.iou(want, gt) and 0 < ev_m["iou"] < 1
    assert ev_m["chamfer"] == ev_w["chamfer"]
    # the key is read only next to evaluation.solver: gpu
    clf = _clf(["iou"], "mesh")
    clf.evaluation.solver = None
    _, ev_off = generate(data, pred, clf)
    assert "iou" not in ev_off


def test_evaluate_reproduces_generate(tmp_path):
    from dgnn_amd.processing.evaluate_mesh import evaluate
    from dgnn_amd.processing.generate_mesh import generate
    g, scene, cen, gt, data = _small_scene(tmp_path)
    mesh, ev = generate(data, torch.from_numpy(g["prediction"]).to(DEV), _clf(["iou", "chamfer"], "mesh"))
    occ_file = os.path.join(str(tmp_path), "eval", "m", "points.npz")
    pc_file = os.path.join(str(tmp_path), "eval", "m", "pointcloud.npz")
    got = evaluate(mesh.vertices, mesh.faces, occ_file=occ_file, pointcloud_file=pc_file, seed=0)
    assert got == ev and set(got) == {"iou", "chamfer"} and np.isfinite(got["chamfer"])
    assert evaluate(mesh.vertices, mesh.faces, occ_file=occ_file) == {"iou": ev["iou"]}
    assert evaluate(mesh.vertices, mesh.faces) == {}
    assert evaluate(mesh.vertices, mesh.faces, pointcloud_file=pc_file, seed=1)["chamfer"] != ev["chamfer"]
