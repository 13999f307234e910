"""`generate` with ``mesh: {solver: gpu, manifold: repair}`` (processing/generate_mesh.py): a noisy sphere scene whose surface
is not watertight as it comes becomes watertight, the repaired labels are the CPU model's, and without the key nothing changes."""
import functools

import numpy as np
import pytest
import torch

import manifold_repair_model as m
import mesh_metrics_model as mm
import mesh_topology_model as mt
from dgnn_amd.config import Config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALE = 1000.0


@functools.lru_cache(maxsize=None)
def _noisy_sphere():
    """800 uniform points, sphere labels with 5 % of the cells inverted -> (scene, signed logit margin sd, labels, neighbours)"""
    scene = mm.scene_from_points(m.uniform_points(800, 1))
    cen = mm.centroids(scene)
    sd = np.linalg.norm(cen - 0.5, axis=1) - 0.3
    sd = np.where(np.random.default_rng(2).random(len(sd)) < 0.05, -sd, sd).astype(np.float32)
    sd[sd == 0] = 1e-3
    labels = (sd > 0).astype(np.int32)
    from scipy.spatial import Delaunay
    nbr = Delaunay(scene["vertices"]).neighbors.astype(np.int32)          # the same call scene_from_points made: the same cells
    return scene, sd, labels, nbr


def _on_disk(tmp_path):
    from test_gpu_mesh_metrics import _write_eval
    scene, sd, labels, _ = _noisy_sphere()
    _write_eval(tmp_path, scene)
    pred = torch.from_numpy(np.stack([-sd, sd], 1)).to(DEV)
    assert np.array_equal(pred.argmax(1).cpu().numpy(), labels)
    data = Config(path=str(tmp_path), gtfile="gt/0", filename="0", id="m", category="", infinite=torch.zeros(len(labels), dtype=torch.int32))
    return data, pred


def _clf(metrics, manifold=None, cost=None, solver="gpu", evaluation=False):
    clf = Config(temp=Config(graph_cut=0, fix_orientation=1, metrics=list(metrics), device=DEV), mesh=Config())
    if solver:
        clf.mesh.solver = solver
    if manifold is not None:
        clf.mesh.manifold = manifold
    if cost is not None:
        clf.mesh.manifold_cost = cost
    if evaluation:
        clf.evaluation = Config(solver="gpu", seed=0)
    return clf


def _margin_cost(sd):
    margin = np.abs(-sd.astype(np.float64) - sd.astype(np.float64)) * SCALE
    return np.minimum(np.rint(margin), 2 ** 20).astype(np.int32)


@pytest.mark.parametrize("cost", ["count", "margin"])
def test_generate_repairs_the_surface(tmp_path, capsys, cost):
    from dgnn_amd.processing.generate_mesh import generate
    scene, sd, labels, nbr = _noisy_sphere()
    nv = len(scene["vertices"])
    assert np.array_equal(mm.scene_from_points(scene["vertices"])["tetrahedra"], scene["tetrahedra"])
    want, st, _, _ = m.repair(scene["tetrahedra"], nbr, labels, nv, cost=None if cost == "count" else _margin_cost(sd))
    assert st["singular_before"] > 0 and st["singular_after"] == 0        # the model shows it first
    data, pred = _on_disk(tmp_path)
    mesh0, ev0 = generate(data, pred, _clf(["watertight"]))
    assert ev0 == {"watertight": 0}                                       # as the labels come, the surface pinches
    mesh, ev = generate(data, pred, _clf(["watertight", "components"], manifold="repair", cost=None if cost == "count" else cost))
    assert ev["watertight"] == 1 and ev["manifold_stuck"] == 0 and ev["manifold_flipped"] == st["flipped_cells"] > 0
    faces, _ = mt.orient_interface(scene, want, mm.interface_ids(want, scene["nfacets"]))
    assert np.array_equal(mesh.vertex_ids[mesh.faces], faces)             # every later stage saw the repaired labels
    assert ev["components"] >= 1 and mt.topology(mesh.faces)["watertight"] == 1
    assert "WARNING" not in capsys.readouterr().out


def test_generate_without_the_key_is_unchanged(tmp_path, capsys):
    from dgnn_amd.processing.generate_mesh import (chamfer_gpu, generate, interface_from_labels, iou_gpu, mesh_components_gpu, mesh_gpu,
                                                   watertight_gpu)
    scene, sd, labels, _ = _noisy_sphere()
    data, pred = _on_disk(tmp_path)
    clf = _clf(["watertight", "components", "iou", "chamfer"], evaluation=True)
    mesh, ev = generate(data, pred, clf)
    lab = torch.from_numpy(labels).to(DEV)
    ids = interface_from_labels(lab, torch.from_numpy(scene["nfacets"]))
    ref = mesh_gpu(scene, lab, ids, 1)
    assert np.array_equal(mesh.faces, ref.faces) and np.array_equal(mesh.vertices, ref.vertices)
    assert ev == {"watertight": watertight_gpu(ref), "components": mesh_components_gpu(ref), "iou": iou_gpu(data, scene, lab),
                  "chamfer": chamfer_gpu(data, scene, ids, clf)}
    assert ev["watertight"] == 0
    assert "WARNING" not in capsys.readouterr().out


def test_generate_reports_stuck_vertices(tmp_path, capsys):
    from dgnn_amd.processing.generate_mesh import generate
    scene, sd, labels, nbr = _noisy_sphere()
    noisy = np.where(np.random.default_rng(5).random(len(sd)) < 0.5, -sd, sd)
    want, st, _, _ = m.repair(scene["tetrahedra"], nbr, (noisy > 0).astype(np.int32), len(scene["vertices"]))
    assert st["singular_after"] > 0
    data, _ = _on_disk(tmp_path)
    pred = torch.from_numpy(np.stack([-noisy, noisy], 1)).to(DEV)
    mesh, ev = generate(data, pred, _clf(["watertight"], manifold="repair"))
    assert ev == {"watertight": 0, "manifold_flipped": st["flipped_cells"], "manifold_stuck": st["singular_after"]}
    out = capsys.readouterr().out
    assert out.count("WARNING") == 1 and "%d vertices of mesh 0 stay non-manifold" % st["singular_after"] in out


def test_generate_refuses_the_key_without_the_gpu_mesh(tmp_path):
    from dgnn_amd.processing.generate_mesh import generate
    data, pred = _on_disk(tmp_path)
    with pytest.raises(ValueError, match="mesh.solver: gpu"):
        generate(data, pred, _clf(["watertight"], manifold="repair", solver=None))
    with pytest.raises(ValueError, match="mesh.manifold"):
        generate(data, pred, _clf(["watertight"], manifold="fix"))
    with pytest.raises(ValueError, match="mesh.manifold_cost"):
        generate(data, pred, _clf(["watertight"], manifold="repair", cost="logit"))
