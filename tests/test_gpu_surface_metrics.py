"""The surface metrics built on the point-to-mesh distance: ops.distance_fold and ops.surface_metrics against the model
tests/mesh_distance_model.py bit for bit and against closed forms, evaluate_mesh.evaluate's new arguments, and generate's new metric names."""
import math
import os

import numpy as np
import pytest
import torch

import mesh_contains_model as mc
import mesh_distance_model as md
import mesh_metrics_model as mm
from dgnn_amd.config import Config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEW_NAMES = ["accuracy", "completeness", "fscore", "normal_consistency", "hausdorff"]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---- the fold ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_distance_fold_equals_the_model(n):
    from dgnn_amd import ops
    rng = np.random.default_rng(n)
    d, c = rng.random(n) * 0.1, rng.uniform(-1, 1, n)
    thresholds = (float(d[n // 2]), 0.05, 0.0, 1.0)                    # the first equals a distance: it counts it
    want = md.fold(d, c, thresholds)
    got = ops.distance_fold(_dev(d), _dev(c), thresholds)
    assert got == want and got[3][0] >= 1 and got[3][3] == n
    assert ops.distance_fold(_dev(d), _dev(c), thresholds) == got          # a rerun: equal bits
    assert ops.distance_fold(_dev(d), None, ()) == (want[0], 0.0, want[2], [])
    assert ops.distance_fold(_dev(d.astype(np.float32)), None, (0.05,)) == md.fold(d.astype(np.float32), None, (0.05,))


def test_distance_fold_of_nothing():
    from dgnn_amd import ops
    assert ops.distance_fold(_dev(np.zeros(0)), None, (1.0,)) == (0.0, 0.0, 0.0, [0])


# ---- surface_metrics -------------------------------------------------------------------------------------------------------------------
def _model_metrics(a, b, samples, thresholds, normals_a, normals_b):
    """the model pipeline on the samples and face normals the device used"""
    s = {k: x.cpu().numpy() for k, x in samples.items()}
    folds = []
    for src, dst, mesh, n_src, n_dst in (("a", "ab", b, normals_a, normals_b), ("b", "ba", a, normals_b, normals_a)):
        d2, face, _, _ = md.distance(mesh[0], mesh[1], s[src + "_points"])
        assert np.array_equal(np.sqrt(d2), s[dst + "_dist"]) and np.array_equal(face, s[dst + "_face"])
        cos = md.row_dot3(n_src, s[src + "_face"], n_dst, face)
        assert np.array_equal(cos, s[dst + "_cosine"])
        folds.append(md.fold(np.sqrt(d2), cos, thresholds))
    return md.metrics_from_folds(folds[0], len(s["a_points"]), folds[1], len(s["b_points"]), thresholds)


def test_surface_metrics_equal_the_model_pipeline():
    from dgnn_amd import ops
    a, b = mc.sphere_interface(300), mc.sphere_interface(400, seed=1)
    thresholds = (0.005, 0.02, 0.1)
    got, samples = ops.surface_metrics(_dev(a[0]), _dev(a[1]), _dev(b[0]), _dev(b[1]), 3000, thresholds, seed=5, return_samples=True)
    na, nb = ops.face_normals(_dev(a[0]), _dev(a[1])).cpu().numpy(), ops.face_normals(_dev(b[0]), _dev(b[1])).cpu().numpy()
    want = _model_metrics(a, b, samples, thresholds, na, nb)
    assert got == want and set(got) == {"accuracy", "completeness", "chamfer_mesh", "hausdorff", "normal_consistency"} | {
        "%s@%g" % (k, t) for k in ("precision", "recall", "fscore") for t in thresholds}
    assert 0 < got["accuracy"] < 0.1 and 0 < got["fscore@0.02"] < 1 and 0 < got["normal_consistency"] <= 1.0
    assert ops.surface_metrics(_dev(a[0]), _dev(a[1]), _dev(b[0]), _dev(b[1]), 3000, thresholds, seed=5) == got          # a rerun
    # the samples are sample_interface's, seed for A and seed + 1 for B
    pa, _ = ops.sample_interface(_dev(a[0]), _dev(a[1]), None, 3000, seed=5)
    pb, _ = ops.sample_interface(_dev(b[0]), _dev(b[1]), None, 3000, seed=6)
    assert torch.equal(pa, samples["a_points"]) and torch.equal(pb, samples["b_points"]) and pa.dtype == torch.float32


def test_surface_metrics_on_concentric_cubes():
    from dgnn_amd import ops
    a, b = mc.cube(0.0, 1.0), mc.cube(-0.1, 1.1)          # B = A scaled by 1.2 about its centre: every point of A is 0.1 from B
    thresholds = (0.0999, 0.1001)
    m, s = ops.surface_metrics(_dev(a[0]), _dev(a[1]), _dev(b[0]), _dev(b[1]), 20000, thresholds, return_samples=True)
    print(m)
    assert abs(m["accuracy"] - 0.1) <= 1e-6 and abs(float(s["ab_dist"].max()) - 0.1) <= 1e-6          # fp32 samples below 1: an ulp is 6e-8
    assert m["precision@0.1001"] == 1.0 and m["precision@0.0999"] == 0.0
    assert 0.1 <= m["completeness"] <= 0.1 * math.sqrt(3)
    assert m["hausdorff"] <= 0.1 * math.sqrt(3) + 1e-6
    assert float(s["ab_cosine"].abs().mean()) >= 0.99          # A's samples face a parallel plane; ties occur only on A's edges
    same = ops.surface_metrics(_dev(a[0]), _dev(a[1]), _dev(a[0]), _dev(a[1]), 20000, (0.01,))
    assert same["accuracy"] < 1e-6 and same["completeness"] < 1e-6 and same["fscore@0.01"] == 1.0


def test_surface_metrics_of_an_empty_mesh(capsys):
    from dgnn_amd import ops
    a = mc.cube(0.0, 1.0)
    flat = np.array([[0, 0, 0], [1, 1, 2]], dtype=np.int32)          # faces without area: nothing to sample
    for args in ((a[0], np.zeros((0, 3), np.int32), a[0], a[1]), (a[0], a[1], a[0], np.zeros((0, 3), np.int32)), (a[0], flat, a[0], a[1])):
        m = ops.surface_metrics(*[_dev(x) for x in args], 100, (0.01,))
        assert m["accuracy"] == m["completeness"] == m["hausdorff"] == m["chamfer_mesh"] == float("inf")
        assert m["fscore@0.01"] == m["precision@0.01"] == m["recall@0.01"] == m["normal_consistency"] == 0.0
        assert "WARNING" in capsys.readouterr().out


# ---- evaluate --------------------------------------------------------------------------------------------------------------------------
def _pointcloud_model(v, f, cloud, thresholds, seed):
    """the pointcloud form on the CPU: GT points -> mesh by all pairs, mesh samples -> GT by fp32 brute force; normals from the device"""
    from dgnn_amd import ops
    gt, nrm = cloud["points"].astype(np.float32), cloud["normals"].astype(np.float64)
    n = len(gt)
    recon, recon_face = (x.cpu().numpy() for x in ops.sample_interface(_dev(v), _dev(f), None, n, seed=seed))
    fn = ops.face_normals(_dev(v), _dev(f)).cpu().numpy()
    d2, face, _, _ = md.distance(v, f, gt)
    d_rc, i_rc = mm.nn_brute(gt, recon)
    fold_gt = md.fold(np.sqrt(d2), md.row_dot3(nrm, np.arange(n), fn, face), thresholds)
    fold_rc = md.fold(d_rc.astype(np.float64), md.row_dot3(fn, recon_face, nrm, i_rc), thresholds)
    return md.metrics_from_folds(fold_rc, n, fold_gt, n, thresholds)


def test_evaluate_with_the_new_arguments(tmp_path):
    from dgnn_amd import ops
    from dgnn_amd.processing.evaluate_mesh import evaluate
    from dgnn_amd.processing.sample_mesh import export_pointcloud
    (v, f), (gv, gf) = mc.sphere_interface(300), mc.sphere_interface(500, seed=2)
    cloud_file = export_pointcloud(gv, gf, os.path.join(str(tmp_path), "pointcloud.npz"), pointcloud_size=1500, seed=3, device=DEV)
    base = evaluate(v, f, pointcloud_file=cloud_file, topology=True, device=DEV)
    assert set(base) == {"chamfer", "components", "largest_component_faces", "watertight"}          # exactly today's keys
    assert set(evaluate(v, f, device=DEV)) == set()
    # a ground-truth mesh
    got = evaluate(v, f, gt_mesh=(gv, gf), thresholds=(0.01, 0.03), n_samples=2000, seed=4, device=DEV)
    assert got == ops.surface_metrics(_dev(v), _dev(f), _dev(gv), _dev(gf), 2000, (0.01, 0.03), seed=4)
    assert "fscore@0.03" in evaluate(v, f, gt_mesh=(gv, gf), n_samples=500, device=DEV, thresholds=(0.03,))
    assert {"fscore@0.01", "fscore@0.02"} <= set(evaluate(v, f, gt_mesh=(gv, gf), n_samples=500, device=DEV))          # the default thresholds
    # the evaluation file's points and normals
    got = evaluate(v, f, pointcloud_file=cloud_file, surface_metrics=True, thresholds=(0.01, 0.03), seed=4, device=DEV)
    want = _pointcloud_model(v, f, np.load(cloud_file), (0.01, 0.03), 4)
    want["chamfer"] = evaluate(v, f, pointcloud_file=cloud_file, seed=4, device=DEV)["chamfer"]
    assert got == want
    assert 0 < got["completeness"] < 0.05 and 0 < got["normal_consistency"] <= 1.0
    with pytest.raises(ValueError):
        evaluate(v, f, surface_metrics=True, device=DEV)


# ---- generate --------------------------------------------------------------------------------------------------------------------------
def _scene(tmp_path, n_points=2500, n_gt=1500):
    rng = np.random.default_rng(3)
    scene = mm.scene_from_points(rng.random((n_points, 3)))
    d = rng.normal(size=(n_gt, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    os.makedirs(os.path.join(str(tmp_path), "eval", "m"), exist_ok=True)
    np.savez(os.path.join(str(tmp_path), "eval", "m", "pointcloud.npz"), points=(0.5 + 0.3 * d).astype(np.float32), normals=d.astype(np.float32))
    os.makedirs(os.path.join(str(tmp_path), "gt"), exist_ok=True)
    np.savez(os.path.join(str(tmp_path), "gt", "0_3dt.npz"), **scene)
    n = len(scene["tetrahedra"])
    sd = np.linalg.norm(mm.centroids(scene) - 0.5, axis=1) - 0.3
    pred = torch.from_numpy(np.stack([-sd, sd], 1).astype(np.float32))
    data = Config(path=str(tmp_path), gtfile="gt/0", filename="0", id="m", category="", infinite=torch.zeros(n, dtype=torch.int32))
    return scene, data, pred, (sd > 0).astype(np.int32)


def _clf(metrics, solver="gpu", mesh_solver=None, thresholds=(0.02, 0.05)):
    clf = Config(temp=Config(graph_cut=0, fix_orientation=1, metrics=metrics, device=DEV))
    if solver:
        clf.evaluation = Config(solver=solver, seed=0, fscore_thresholds=list(thresholds))
    if mesh_solver:
        clf.mesh = Config(solver=mesh_solver)
    return clf


def _expected_keys(thresholds):
    return {"accuracy", "completeness", "hausdorff", "normal_consistency", "fscore"} | {"%s@%g" % (k, t) for k in ("precision", "recall", "fscore")
                                                                                       for t in thresholds}


def test_generate_fills_the_surface_metrics(tmp_path, capsys):
    from dgnn_amd.processing.evaluate_mesh import evaluate
    from dgnn_amd.processing.generate_mesh import generate
    scene, data, pred, labels = _scene(tmp_path)
    cloud_file = os.path.join(str(tmp_path), "eval", "m", "pointcloud.npz")
    # mesh.solver: gpu -- on the exported faces
    mesh, ev = generate(data, pred.to(DEV), _clf(NEW_NAMES, mesh_solver="gpu"))
    assert set(ev) == _expected_keys((0.02, 0.05))
    want = evaluate(mesh.vertices, mesh.faces, pointcloud_file=cloud_file, surface_metrics=True, thresholds=(0.02, 0.05), seed=0, device=DEV)
    assert all(ev[k] == want[k] for k in ev if k != "fscore") and ev["fscore"] == want["fscore@0.02"]
    assert 0 < ev["accuracy"] < 0.05 and 0 < ev["completeness"] < 0.05 and 0.5 < ev["normal_consistency"] <= 1 and 0 < ev["fscore@0.05"] <= 1
    # without it -- on the interface facets
    ids = mm.interface_ids(labels, scene["nfacets"])
    _, ev2 = generate(data, pred.to(DEV), _clf(["hausdorff", "fscore"], thresholds=(0.05,)))
    want2 = evaluate(scene["vertices"], scene["facets"][ids], pointcloud_file=cloud_file, surface_metrics=True, thresholds=(0.05,), seed=0, device=DEV)
    assert ev2 == {k: want2[k] for k in ("hausdorff", "fscore@0.05", "precision@0.05", "recall@0.05")} | {"fscore": want2["fscore@0.05"]}
    assert "WARNING" not in capsys.readouterr().out
    # the default thresholds
    clf = _clf(["fscore"])
    clf.evaluation = Config(solver="gpu", seed=0)
    assert set(generate(data, pred.to(DEV), clf)[1]) == {"fscore"} | {"%s@%g" % (k, t) for k in ("precision", "recall", "fscore") for t in (0.01, 0.02)}
    # absent without the gpu solver
    _, ev3 = generate(data, pred.to(DEV), _clf(NEW_NAMES, solver=None, mesh_solver="gpu"))
    assert not set(ev3) & _expected_keys((0.02, 0.05))
    capsys.readouterr()
    # a failure: the reference's style of warning, inf for the distances and 0.0 for the scores
    os.remove(cloud_file)
    _, ev4 = generate(data, pred.to(DEV), _clf(NEW_NAMES))
    assert ev4 == dict({"accuracy": float("inf"), "completeness": float("inf"), "hausdorff": float("inf"), "normal_consistency": 0.0, "fscore": 0.0},
                       **{"%s@%g" % (k, t): 0.0 for k in ("precision", "recall", "fscore") for t in (0.02, 0.05)})
    assert set(ev4) == _expected_keys((0.02, 0.05))          # the key set does not depend on whether the computation failed
    assert "WARNING: Could not calculate surface metrics for mesh" in capsys.readouterr().out


@pytest.mark.parametrize("mesh_solver", [None, "gpu"])
def test_generate_empty_interface_takes_the_warning_path(tmp_path, capsys, mesh_solver):
    from dgnn_amd.processing.generate_mesh import generate
    scene, data, pred, _ = _scene(tmp_path, n_points=400, n_gt=100)
    pred = torch.zeros(len(pred), 2)
    pred[:, 1] = 1.0                                               # every cell outside: no interface
    mesh, ev = generate(data, pred.to(DEV), _clf(NEW_NAMES, mesh_solver=mesh_solver))
    assert len(np.asarray(mesh.faces)) == 0
    assert ev["accuracy"] == ev["completeness"] == ev["hausdorff"] == float("inf")
    assert ev["fscore"] == ev["normal_consistency"] == ev["fscore@0.02"] == ev["recall@0.05"] == 0.0
    assert "has no faces" in capsys.readouterr().out
