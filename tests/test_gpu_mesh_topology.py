"""The device mesh of `generate` with ``mesh.solver: gpu`` (ops.orient_interface / compact_vertices / mesh_topology,
generate_mesh.mesh_gpu / watertight_gpu) against the CPU model tests/mesh_topology_model.py: exact orientation signs (fp64 with a loose
bound, Fractions elsewhere), np.unique compaction, dictionary edge and vertex counts."""
import os

import numpy as np
import pytest
import torch

import mesh_metrics_model as mm
import mesh_topology_model as mt
from dgnn_amd.config import Config
from helpers import gold

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gold_scene():
    g = gold("genmesh_f4_small.npz")
    scene = {k: g[k] for k in ("vertices", "tetrahedra", "facets", "nfacets")}
    labels = np.argmax(g["prediction"][g["infinite"] == 0], axis=1).astype(np.int32)     # ties -> inside, as dgnn_argmax_rows
    return scene, labels, g


def _case(which):
    if which == "genmesh_f4_small":
        scene, labels, _ = _gold_scene()
        return scene, labels
    if which.startswith("grid"):
        scene = mt.regular_grid_scene()
        n = len(scene["tetrahedra"])
        if which == "grid_sphere":
            return scene, mm.sphere_labels(scene, center=scene["vertices"].mean(0), radius=0.3 * 7.3 * 9)
        return scene, (np.random.default_rng(4).random(n) > 0.1).astype(np.int32)
    scene = mm.random_scene(20000, seed=3)
    n = len(scene["tetrahedra"])
    if which == "random_sphere":
        return scene, mm.sphere_labels(scene)
    return scene, (np.random.default_rng(5).random(n) > 0.1).astype(np.int32)


def _orient(scene, labels, ids, **kw):
    from dgnn_amd import ops
    return ops.orient_interface(scene["vertices"], scene["tetrahedra"], scene["facets"], scene["nfacets"], torch.from_numpy(labels).to(DEV),
                                torch.from_numpy(np.asarray(ids, dtype=np.int32)).to(DEV), **kw)


def _topology(faces, nv):
    from dgnn_amd import ops
    return ops.mesh_topology(torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).to(DEV), nv)


CASES = ["genmesh_f4_small", "random_sphere", "random_10pct", "grid_sphere", "grid_10pct"]


# ---- orientation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CASES)
def test_orientation_is_bit_equal_to_the_oracle(which):
    scene, labels = _case(which)
    ids = mm.interface_ids(labels, scene["nfacets"])
    assert len(ids) > 0
    faces, und, exact_used = _orient(scene, labels, ids, return_exact_used=True)
    want, want_und = mt.orient_interface(scene, labels, ids)
    assert np.array_equal(faces.cpu().numpy(), want) and und == want_und
    if which.startswith("grid"):
        # the exact stage is needed here: plain fp64 gets the sign of some facet's inside-cell vertex wrong
        fac = scene["facets"][ids].astype(np.int64)
        cells = scene["nfacets"][ids].astype(np.int64)
        lab = np.append(labels, 1)
        inside = lab[np.where(cells < 0, len(labels), cells)] == 0
        ci = np.where(inside[:, 0], cells[:, 0], cells[:, 1])
        t = scene["tetrahedra"][ci].astype(np.int64)
        d = t[~(t[:, :, None] == fac[:, None, :]).any(axis=2)]
        v = scene["vertices"]
        p = (v[fac[:, 0]], v[fac[:, 1]], v[fac[:, 2]], v[d])
        assert (mt.naive_sign(*p) != mt.orient_sign(*p)).any()
        assert exact_used
    faces0, und0 = _orient(scene, labels, ids, orient=False)           # fix_orientation off: the stored winding
    assert np.array_equal(faces0.cpu().numpy(), scene["facets"][ids]) and und0 == 0


def test_flat_cells_fall_back_and_are_counted():
    # an unrotated grid: flat cells have exactly zero orientation; between two flat cells or a flat cell and the infinite one the
    # winding stays as stored and is counted
    g = np.stack(np.meshgrid(*(np.arange(6, dtype=np.float64),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    scene = mm.scene_from_points(g)
    labels = (np.random.default_rng(2).random(len(scene["tetrahedra"])) > 0.3).astype(np.int32)
    ids = mm.interface_ids(labels, scene["nfacets"])
    faces, und = _orient(scene, labels, ids)
    want, want_und = mt.orient_interface(scene, labels, ids)
    assert np.array_equal(faces.cpu().numpy(), want) and und == want_und


@pytest.mark.parametrize("which", CASES)
def test_topology_counts_equal_the_oracle(which):
    scene, labels = _case(which)
    ids = mm.interface_ids(labels, scene["nfacets"])
    faces, _ = mt.orient_interface(scene, labels, ids)
    assert _topology(faces, len(scene["vertices"])) == mt.topology(faces)
    stored = scene["facets"][ids]
    assert _topology(stored, len(scene["vertices"])) == mt.topology(stored)


@pytest.mark.parametrize("case", ["tet", "vertex", "edge", "open", "empty"])
def test_topology_of_hand_made_meshes(case):
    faces = {"tet": mt.tetra_faces((0, 1, 2, 3)), "vertex": mt.tetra_faces((0, 1, 2, 3)) + mt.tetra_faces((3, 5, 6, 7)),
             "edge": mt.tetra_faces((0, 1, 2, 3)) + mt.tetra_faces((0, 1, 6, 7)), "open": mt.tetra_faces((0, 1, 2, 3))[:3],
             "empty": []}[case]
    faces = np.array(faces, dtype=np.int32).reshape(-1, 3)
    got = _topology(faces, 9)
    assert got == mt.topology(faces)
    assert got["watertight"] == (case == "tet")
    if case == "vertex":
        assert got["nonmanifold_vertices"] == 1 and got["nonmanifold_edges"] == 0
    if case == "edge":
        assert got["nonmanifold_edges"] == 1 and got["nonmanifold_vertices"] == 0


def test_topology_with_edge_keys_just_above_a_tile_of_the_sort():
    """683 faces: 3 F = 2049 edge keys and 6 F = 4098 link keys, each one element into a new 2048-element tile of the radix sort
    (RX_TILE of csrc/reorder.hip), where the histogram count of the sort's workspace steps"""
    rng = np.random.default_rng(683)
    faces = np.stack([rng.permutation(200)[:3] for _ in range(683)]).astype(np.int32)          # a soup: every face has three distinct vertices
    assert 3 * len(faces) == 2048 + 1
    assert _topology(faces, 200) == mt.topology(faces)


def test_generic_scene_encloses_the_inside_volume():
    scene = mm.random_scene(5000, seed=11)
    labels = mm.sphere_labels(scene)
    ids = mm.interface_ids(labels, scene["nfacets"])
    faces, und = _orient(scene, labels, ids)
    f = faces.cpu().numpy()
    assert und == 0 and _topology(f, len(scene["vertices"]))["winding_mismatch_edges"] == 0
    want = mt.inside_volume(scene, labels)
    assert abs(mt.signed_volume(scene["vertices"], f) - want) <= 1e-9 * want


def test_compaction_matches_the_oracle_and_reruns_are_bit_identical():
    from dgnn_amd import ops
    scene, labels = _case("random_10pct")
    ids = mm.interface_ids(labels, scene["nfacets"])
    runs = []
    for _ in range(3):
        faces, und = _orient(scene, labels, ids)
        fc, kept = ops.compact_vertices(faces, len(scene["vertices"]))
        runs.append((faces.cpu().numpy(), und, fc.cpu().numpy(), kept.cpu().numpy(), ops.mesh_topology(fc, len(kept))))
    want_fc, want_kept = mt.compact(runs[0][0])
    assert np.array_equal(runs[0][2], want_fc) and np.array_equal(runs[0][3], want_kept)
    assert runs[0][4] == mt.topology(want_fc)
    for r in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(r[:4], runs[0][:4])) and r[4] == runs[0][4]


def test_invalid_input_raises():
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    scene, labels = _case("genmesh_f4_small")
    ids = mm.interface_ids(labels, scene["nfacets"])
    _orient(scene, labels, ids)
    with pytest.raises(DgnnError, match="out of range"):
        _orient(scene, labels, np.append(ids, len(scene["facets"])))
    not_interface = np.setdiff1d(np.arange(len(scene["facets"])), ids)[:1]
    with pytest.raises(DgnnError, match="does not separate"):
        _orient(scene, labels, np.append(ids, not_interface))
    bad = dict(scene, facets=scene["facets"].copy())
    f = int(ids[0])
    bad["facets"][f, 0] = next(x for x in range(len(scene["vertices"])) if x not in scene["facets"][f])
    with pytest.raises(DgnnError, match="not a face"):
        _orient(bad, labels, ids)
    repeated = dict(vertices=np.eye(4, 3), tetrahedra=np.array([[0, 0, 1, 3]], dtype=np.int32), facets=np.array([[0, 1, 2]], dtype=np.int32),
                    nfacets=np.array([[0, -1]], dtype=np.int32))          # three slots of the cell on the facet, and the facet's vertex 2 missing
    with pytest.raises(DgnnError, match="not a face"):
        _orient(repeated, np.zeros(1, dtype=np.int32), [0])
    bad = dict(scene, vertices=scene["vertices"].copy())
    bad["vertices"][scene["facets"][f, 1], 2] = np.nan
    with pytest.raises(DgnnError, match="non-finite"):
        _orient(bad, labels, ids)
    faces = np.array(mt.tetra_faces((0, 1, 2, 3)), dtype=np.int32)
    with pytest.raises(DgnnError, match="out of range"):
        _topology(faces, 3)
    with pytest.raises(DgnnError, match="repeated vertex"):
        _topology(np.array([[0, 1, 1]], dtype=np.int32), 4)
    with pytest.raises(DgnnError, match="out of range"):
        ops.compact_vertices(torch.from_numpy(faces).to(DEV), 3)


@pytest.fixture
def current_device_calls(monkeypatch):
    """Records every call of torch.cuda.current_device() made from the package (the work must go where the tensors are)."""
    import inspect
    real = torch.cuda.current_device
    calls = []

    def spy():
        caller = inspect.stack()[1].filename
        if os.sep + "dgnn_amd" + os.sep in caller:
            calls.append(caller)
        return real()
    monkeypatch.setattr(torch.cuda, "current_device", spy)
    return calls


def test_runs_on_the_device_of_its_inputs(current_device_calls):
    from dgnn_amd.processing.generate_mesh import mesh_gpu, watertight_gpu
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    scene, labels = _case("random_sphere")
    ids = mm.interface_ids(labels, scene["nfacets"])
    dev = torch.device("cuda:1")
    assert torch.cuda.current_device() == 0
    current_device_calls.clear()
    mesh = mesh_gpu(scene, torch.from_numpy(labels).to(dev), torch.from_numpy(ids).to(dev), True)
    wt = watertight_gpu(mesh)
    assert mesh.faces_dev.device == dev and current_device_calls == []
    want, _ = mt.orient_interface(scene, labels, ids)
    assert np.array_equal(mesh.vertex_ids[mesh.faces], want) and wt == mt.topology(want)["watertight"]


def test_million_tet_scene_against_the_oracle():
    from dgnn_amd import ops
    scene = mm.random_scene(170000, seed=21)
    assert len(scene["tetrahedra"]) > 1_000_000
    labels = mm.sphere_labels(scene)
    ids = mm.interface_ids(labels, scene["nfacets"])
    faces, und = _orient(scene, labels, ids)
    want, want_und = mt.orient_interface(scene, labels, ids)
    assert np.array_equal(faces.cpu().numpy(), want) and und == want_und
    fc, kept = ops.compact_vertices(faces, len(scene["vertices"]))
    want_fc, want_kept = mt.compact(want)
    assert np.array_equal(fc.cpu().numpy(), want_fc) and np.array_equal(kept.cpu().numpy(), want_kept)
    assert ops.mesh_topology(fc, len(kept)) == mt.topology(want_fc)


# ---- generate ---------------------------------------------------------------------------------------------------------------------
def _generate_data(tmp_path, g):
    os.makedirs(os.path.join(str(tmp_path), "gt"), exist_ok=True)
    np.savez(os.path.join(str(tmp_path), "gt", "0_3dt.npz"), vertices=g["vertices"], tetrahedra=g["tetrahedra"], facets=g["facets"], nfacets=g["nfacets"])
    return Config(path=str(tmp_path), gtfile="gt/0", filename="0", id="", category="", infinite=torch.from_numpy(g["infinite"]))


def _mesh_clf(fix, metrics=(), solver="gpu"):
    clf = Config(temp=Config(graph_cut=0, fix_orientation=fix, metrics=list(metrics), device=DEV))
    if solver is not None:
        clf.mesh = Config(solver=solver)
    return clf


def _read_ply(path):
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    head = blob[:end].decode().split("\n")
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in head if h.startswith("element face")).split()[-1])
    v = np.frombuffer(blob, dtype="<f8", count=3 * nv, offset=end).reshape(nv, 3)
    rec = np.frombuffer(blob, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=end + 24 * nv)
    assert (rec["n"] == 3).all()
    return v, rec["i"]


@pytest.mark.parametrize("fix", [0, 1])
def test_generate_builds_the_mesh_on_the_gpu(tmp_path, capsys, fix):
    from dgnn_amd.processing.generate_mesh import InterfaceMesh, generate
    scene, labels, g = _gold_scene()
    data = _generate_data(tmp_path, g)
    mesh, ev = generate(data, torch.from_numpy(g["prediction"]).to(DEV), _mesh_clf(fix, ["watertight"]))
    assert isinstance(mesh, InterfaceMesh) and mesh.faces.shape == g["faces"].shape
    ids = mm.interface_ids(labels, scene["nfacets"])
    want = g["faces"] if fix == 0 else mt.orient_interface(scene, labels, ids)[0]
    assert np.array_equal(mesh.vertex_ids[mesh.faces], want)
    assert np.array_equal(mesh.vertices, g["vertices"][mesh.vertex_ids]) and np.array_equal(mesh.vertex_ids, np.unique(want))
    want_fc, _ = mt.compact(want)
    assert ev == {"watertight": mt.topology(want_fc)["watertight"]}
    if fix:
        assert not np.array_equal(want, g["faces"])        # the fixture's stored winding is mixed: the test sees the orientation
    v, f = _read_ply(mesh.export(os.path.join(str(tmp_path), "m.ply")))
    assert np.array_equal(v, mesh.vertices) and np.array_equal(f, mesh.faces)
    assert "WARNING" not in capsys.readouterr().out
    # without the key: today's mesh
    mesh0, ev0 = generate(data, torch.from_numpy(g["prediction"]).to(DEV), _mesh_clf(fix, [], solver=None))
    assert ev0 == {} and np.array_equal(np.asarray(mesh0.faces), g["faces"]) and np.array_equal(np.asarray(mesh0.vertices), g["vertices_out"])


def test_generate_combines_with_the_gpu_metrics_and_graph_cut(tmp_path, capsys):
    from dgnn_amd.processing.generate_mesh import generate
    from test_gpu_mesh_metrics import _write_eval
    rng = np.random.default_rng(3)
    scene = mm.scene_from_points(rng.random((3000, 3)))
    _write_eval(tmp_path, scene)
    n = len(scene["tetrahedra"])
    sd = np.linalg.norm(mm.centroids(scene) - 0.5, axis=1) - 0.3
    pred = torch.from_numpy(np.stack([-sd, sd], 1).astype(np.float32)).to(DEV)
    data = Config(path=str(tmp_path), gtfile="gt/0", filename="0", id="m", category="", infinite=torch.zeros(n, dtype=torch.int32))
    clf = _mesh_clf(1, ["watertight", "iou", "chamfer"])
    clf.evaluation = Config(solver="gpu", seed=0)
    mesh, ev = generate(data, pred, clf)
    clf_metrics = _mesh_clf(1, ["iou", "chamfer"], solver=None)
    clf_metrics.evaluation = Config(solver="gpu", seed=0)
    _, ev_metrics = generate(data, pred, clf_metrics)
    labels = (sd > 0).astype(np.int32)
    want, _ = mt.orient_interface(scene, labels, mm.interface_ids(labels, scene["nfacets"]))
    assert np.array_equal(mesh.vertex_ids[mesh.faces], want)
    assert ev["iou"] == ev_metrics["iou"] and ev["chamfer"] == ev_metrics["chamfer"]
    assert ev["watertight"] == mt.topology(want)["watertight"]
    clf.temp.graph_cut = 1
    clf.graph_cut = Config(unary_weight=10.0, binary_weight=1.0, binary_type=0, solver="gpu")
    mesh_gc, ev_gc = generate(data, pred, clf)
    assert set(ev_gc) == {"watertight", "iou", "chamfer"} and len(mesh_gc.faces) > 0
    assert "WARNING" not in capsys.readouterr().out


def test_generate_empty_interface_is_not_watertight(tmp_path, capsys):
    from dgnn_amd.processing.generate_mesh import generate
    _, _, g = _gold_scene()
    data = _generate_data(tmp_path, g)
    pred = torch.zeros(len(g["prediction"]), 2)
    pred[:, 1] = 1.0
    mesh, ev = generate(data, pred.to(DEV), _mesh_clf(1, ["watertight"]))
    assert len(mesh.faces) == 0 and len(mesh.vertices) == 0 and ev == {"watertight": 0}
    assert "has no faces" in capsys.readouterr().out
