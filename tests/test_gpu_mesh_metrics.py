"""The device mesh metrics (ops.locate_points / iou_counts / mesh_iou / sample_interface / nearest_neighbor / chamfer_distance,
generate_mesh.iou_gpu / chamfer_gpu, `evaluation.solver: gpu` in generate and Trainer.train_test) against the CPU model
tests/mesh_metrics_model.py: brute-force containment, scipy's find_simplex, the sampler restatement, fp32 brute-force and cKDTree
nearest neighbours."""
import os

import numpy as np
import pytest
import torch

import mesh_metrics_model as mm
from dgnn_amd.config import Config
from helpers import gold

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _locate(scene, q, **kw):
    from dgnn_amd import ops
    out = ops.locate_points(scene["vertices"], scene["tetrahedra"], scene["facets"], scene["nfacets"], torch.from_numpy(q).to(DEV), **kw)
    return (out[0].cpu().numpy(), out[1]) if kw.get("return_steps") else out.cpu().numpy()


def _gold_scene():
    g = gold("genmesh_f4_small.npz")
    return {k: g[k] for k in ("vertices", "tetrahedra", "facets", "nfacets")}, g


# ---- point location -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["genmesh_f4_small", "random40", "random120"])
def test_location_matches_brute_force_containment(which):
    scene = _gold_scene()[0] if which == "genmesh_f4_small" else mm.random_scene(int(which[6:]), seed=len(which))
    v = scene["vertices"]
    lo, hi = v.min(0), v.max(0)
    rng = np.random.default_rng(1)
    q = (lo + (rng.random((3000, 3)) * 1.2 - 0.1) * (hi - lo)).astype(np.float32)
    cells = _locate(scene, q)
    inside = mm.brute_containing(scene, q)
    holds = inside.any(axis=1)
    assert holds.any() and (~holds).any()
    assert np.array_equal(cells >= 0, holds)
    assert inside[np.nonzero(cells >= 0)[0], cells[cells >= 0]].all()


@pytest.mark.parametrize("n_points", [200, 3000, 30000, 150000])
def test_location_matches_find_simplex(n_points):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(n_points)
    pts = rng.random((n_points, 3)).astype(np.float32).astype(np.float64)    # vertices exact in fp32: hull vertices are queried as they are
    scene = mm.scene_from_points(pts)
    hull = pts[np.unique(Delaunay(pts).convex_hull)][:500].astype(np.float32)        # on the hull (vertices)
    q = np.concatenate([(rng.random((100000, 3)) * 1.1 - 0.05).astype(np.float32), hull])
    cells, steps = _locate(scene, q, return_steps=True)
    s = Delaunay(pts).find_simplex(q.astype(np.float64))
    clear = s >= 0
    assert np.array_equal(cells[:100000] >= 0, s[:100000] >= 0)
    # a point on the hull is on the boundary: it gets a cell that holds it (checked below) or -1 (outside); qhull's hull is convex only up
    # to rounding, so which one is not fixed here
    found = cells >= 0
    assert mm.cell_signs(scene, cells[found], q[found]).all()
    agree = (cells == s)[:100000][clear[:100000]].mean()
    assert agree > 0.999                                 # only points on shared faces may differ, and then both cells hold them
    assert 0 < steps < 65536


def test_points_on_shared_faces_and_vertices_follow_the_rule():
    scene = mm.scene_from_points(np.random.default_rng(11).random((300, 3)).astype(np.float32).astype(np.float64))
    v, t, f, nf = scene["vertices"], scene["tetrahedra"], scene["facets"], scene["nfacets"]
    inner = np.nonzero(nf[:, 1] >= 0)[0][:400]
    on_hull = np.unique(f[nf[:, 1] < 0])
    interior = np.setdiff1d(np.arange(len(v)), on_hull)[:200]
    # facet centroids (on the face up to fp32 rounding) and interior vertices (exactly shared by many cells)
    q = np.concatenate([v[f[inner]].mean(axis=1), v[interior]]).astype(np.float32)
    cells = _locate(scene, q)
    assert (cells >= 0).all()
    found = cells >= 0
    assert mm.cell_signs(scene, cells[found], q[found]).all()     # a cell whose four signs are >= 0
    again = _locate(scene, q)
    assert np.array_equal(cells, again)


def test_location_rerun_is_bit_identical_and_resolves_under_the_cap():
    scene = mm.random_scene(150000, seed=0)
    q = np.random.default_rng(2).random((400000, 3)).astype(np.float32)
    a, sa = _locate(scene, q, return_steps=True)
    b, sb = _locate(scene, q, return_steps=True)
    assert np.array_equal(a, b) and sa == sb and sa < 65536


def test_location_errors_raise():
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    scene = mm.random_scene(50, seed=1)
    q = torch.rand(10, 3, device=DEV)
    bad = dict(scene, tetrahedra=scene["tetrahedra"].copy())
    bad["tetrahedra"][3, 1] = len(scene["vertices"])
    nonfinite = dict(scene, vertices=scene["vertices"].copy())
    nonfinite["vertices"][5, 2] = np.inf
    badcell = dict(scene, nfacets=scene["nfacets"].copy())
    badcell["nfacets"][4, 0] = len(scene["tetrahedra"])
    swapped = dict(scene, nfacets=scene["nfacets"].copy())
    i = np.nonzero(swapped["nfacets"][:, 1] >= 0)[0][0]
    swapped["nfacets"][i, 1] = (swapped["nfacets"][i, 1] + 7) % len(scene["tetrahedra"])
    missing = dict(scene, facets=scene["facets"][1:], nfacets=scene["nfacets"][1:])
    for s in (bad, nonfinite, badcell, swapped, missing):
        with pytest.raises(DgnnError):
            ops.locate_points(s["vertices"], s["tetrahedra"], s["facets"], s["nfacets"], q)
    with pytest.raises(DgnnError):
        ops.locate_points(scene["vertices"], scene["tetrahedra"], scene["facets"], scene["nfacets"], torch.full((3, 3), float("nan"), device=DEV))
    with pytest.raises(DgnnError):          # the cell repeats a vertex and lacks the facet's vertex 2: the facet is no face of it
        ops.locate_points(np.eye(4, 3), np.array([[0, 0, 1, 3]], dtype=np.int32), np.array([[0, 1, 2]], dtype=np.int32),
                          np.array([[0, -1]], dtype=np.int32), q)
    assert len(_locate(scene, np.random.default_rng(0).random((5, 3)).astype(np.float32))) == 5


# ---- IoU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labelling", ["sphere", "all_inside", "all_outside", "graph_cut"])
def test_iou_counts_equal_the_oracle(labelling):
    from dgnn_amd import ops
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(7)
    pts = rng.random((20000, 3))
    scene = mm.scene_from_points(pts)
    n = len(scene["tetrahedra"])
    if labelling == "sphere":
        labels = mm.sphere_labels(scene)
    elif labelling == "all_inside":
        labels = np.zeros(n, np.int32)
    elif labelling == "all_outside":
        labels = np.ones(n, np.int32)
    else:
        import graph_cut_model as gcm
        cent = mm.centroids(scene)
        nf = scene["nfacets"]
        lab, _, _ = ops.binary_graph_cut(torch.from_numpy(gcm.coherent_logits(cent, seed=3)).to(DEV),
                                         torch.from_numpy(nf[(nf >= 0).all(1)]).to(DEV), 10, 10)
        labels = lab.cpu().numpy()
    q = (rng.random((100000, 3)) * 1.1 - 0.05).astype(np.float32)
    gt = np.linalg.norm(q - 0.52, axis=1) < 0.31
    iou, occ, inter, union = ops.mesh_iou(scene["vertices"], scene["tetrahedra"], scene["facets"], scene["nfacets"], torch.from_numpy(labels), q, gt)
    s = Delaunay(pts).find_simplex(q.astype(np.float64))
    want_occ = (s >= 0) & (labels[np.maximum(s, 0)] == 0)
    occ = occ.cpu().numpy().astype(bool)
    cells = _locate(scene, q)
    exact = (occ == ((cells >= 0) & (labels[np.maximum(cells, 0)] == 0)))
    assert exact.all()
    assert (occ != want_occ).sum() <= 2                  # points on a face between differently labelled cells only
    assert inter == int((occ & gt).sum()) and union == int((occ | gt).sum())
    want = mm.iou(occ, gt)
    assert iou == want or (np.isnan(iou) and np.isnan(want))
    if labelling == "all_outside":
        assert inter == 0 and iou == 0.0


# ---- sampler --------------------------------------------------------------------------------------------------------------------
def _interface_scene(n_points=20000, seed=0):
    scene = mm.random_scene(n_points, seed=seed)
    labels = mm.sphere_labels(scene)
    return scene, labels, mm.interface_ids(labels, scene["nfacets"])


def test_sampler_matches_the_restatement():
    from dgnn_amd import ops
    scene, _, ids = _interface_scene()
    for seed, n in ((0, 100000), (12345, 777), (2 ** 63 + 5, 1)):
        pts, face, cum = ops.sample_interface(scene["vertices"], scene["facets"], torch.from_numpy(ids).to(DEV), n, seed=seed, return_cum=True)
        cum = cum.cpu().numpy()
        want_cum = np.cumsum(mm.face_areas(scene["vertices"], scene["facets"], ids))
        assert np.abs(cum - want_cum).max() <= 1e-12 * want_cum[-1]
        want_p, want_j = mm.sample(scene["vertices"], scene["facets"], ids, cum, n, seed)
        assert np.array_equal(pts.cpu().numpy(), want_p) and np.array_equal(face.cpu().numpy(), want_j)


def test_sampler_counts_follow_area_and_samples_lie_on_their_faces():
    from scipy.stats import chisquare
    from dgnn_amd import ops
    scene, _, ids = _interface_scene(3000, seed=2)
    f = scene["facets"].copy()
    f[ids[::5], 2] = f[ids[::5], 1]                      # every fifth face degenerate: zero area, no samples
    n = 400000
    pts, face = ops.sample_interface(scene["vertices"], f, ids, n, seed=4)
    pts, face = pts.cpu().numpy(), face.cpu().numpy()
    areas = mm.face_areas(scene["vertices"], f, ids)
    counts = np.bincount(face, minlength=len(ids))
    assert counts[areas == 0].sum() == 0
    pos = areas > 0
    assert chisquare(counts[pos], areas[pos] / areas.sum() * n).pvalue > 1e-3
    v = scene["vertices"][f[ids[face]]]
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    off = np.abs(np.einsum("ij,ij->i", pts - v[:, 0], nrm)) / np.linalg.norm(nrm, axis=1)
    assert off.max() < 1e-6
    # inside the triangle: barycentric coordinates >= 0 up to fp32 rounding
    e1, e2, w = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], pts - v[:, 0]
    d00, d01, d11 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    d20, d21 = (w * e1).sum(1), (w * e2).sum(1)
    den = d00 * d11 - d01 * d01
    b1, b2 = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
    assert b1.min() > -1e-4 and b2.min() > -1e-4 and (b1 + b2).max() < 1 + 1e-4


def test_sampler_errors_raise():
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    scene, _, ids = _interface_scene(300, seed=3)
    with pytest.raises(DgnnError):
        ops.sample_interface(scene["vertices"], scene["facets"], np.array([len(scene["facets"])], np.int32), 10)
    flat = scene["facets"].copy()
    flat[:, 2] = flat[:, 1]
    with pytest.raises(DgnnError):
        ops.sample_interface(scene["vertices"], flat, ids, 10)


# ---- nearest neighbour ----------------------------------------------------------------------------------------------------------
def _nn(ref, q):
    from dgnn_amd import ops
    d, i, s = ops.nearest_neighbor(torch.from_numpy(ref).to(DEV), torch.from_numpy(q).to(DEV))
    return d.cpu().numpy(), i.cpu().numpy(), s


def _surface(n, rng, r=0.3):
    p = rng.normal(size=(n, 3))
    return (0.5 + r * p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)


NN_SEEDS = {"uniform": 11, "surface": 12, "duplicates": 13, "one_point": 14, "unequal": 15, "far": 16, "flat": 17}


@pytest.mark.parametrize("case", list(NN_SEEDS))
def test_nearest_neighbour_is_bit_equal_to_brute_force(case):
    rng = np.random.default_rng(NN_SEEDS[case])
    if case == "uniform":
        ref, q = rng.random((8000, 3)).astype(np.float32), rng.random((10000, 3)).astype(np.float32)
    elif case == "surface":
        ref, q = _surface(10000, rng), _surface(7000, rng, r=0.31)
    elif case == "duplicates":
        base = rng.random((300, 3)).astype(np.float32)
        ref = base[rng.integers(0, 300, 6000)]
        q = np.concatenate([base, rng.random((3000, 3)).astype(np.float32)])
    elif case == "one_point":
        ref, q = rng.random((1, 3)).astype(np.float32), rng.random((5000, 3)).astype(np.float32)
    elif case == "unequal":
        ref, q = rng.random((10000, 3)).astype(np.float32), rng.random((7, 3)).astype(np.float32)
        d, i, _ = _nn(q, ref)                                        # and the other way round: 7 reference points, 10 000 queries
        wd, wi = mm.nn_brute(q, ref)
        assert np.array_equal(d, wd) and np.array_equal(i, wi)
    elif case == "far":
        ref, q = rng.random((5000, 3)).astype(np.float32), (rng.random((2000, 3)) * 40 - 20).astype(np.float32)
    else:
        ref = rng.random((6000, 3)).astype(np.float32)
        ref[:, 2] = 0.25                                              # a flat set: one bin along z
        q = rng.random((4000, 3)).astype(np.float32)
    d, i, s = _nn(ref, q)
    wd, wi = mm.nn_brute(ref, q)
    assert np.array_equal(d, wd) and np.array_equal(i, wi)
    assert abs(s - wd.astype(np.float64).sum()) <= 1e-12 * max(1.0, s)
    assert _nn(ref, q)[2] == s                                       # the fixed-order sum is bit-identical from run to run


@pytest.mark.parametrize("n", [100000, 1000000])
def test_nearest_neighbour_matches_ckdtree(n):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(n)
    ref = _surface(n, rng)
    q = _surface(n // 2, rng, r=0.305)
    d, i, _ = _nn(ref, q)
    wd, _ = cKDTree(ref).query(q)
    assert np.abs(d - wd).max() <= 1e-6 * np.abs(wd).max() + 1e-7
    rel = np.abs(d - wd) / np.maximum(wd, 1e-30)
    assert np.median(rel) < 1e-6


def test_chamfer_matches_the_ckdtree_formula():
    from dgnn_amd import ops
    rng = np.random.default_rng(5)
    gt, rc = _surface(100000, rng), _surface(100000, rng, r=0.302)
    got = ops.chamfer_distance(torch.from_numpy(gt).to(DEV), torch.from_numpy(rc).to(DEV))
    want = mm.chamfer_ckdtree(gt, rc)
    assert abs(got - want) <= 1e-6 * want
    assert ops.chamfer_distance(torch.from_numpy(gt).to(DEV), torch.from_numpy(rc).to(DEV)) == got


# ---- generate and train_test ----------------------------------------------------------------------------------------------------
def _write_eval(tmp_path, scene, n_gt=5000, sub="m"):
    rng = np.random.default_rng(9)
    q = (rng.random((3001, 3)) * 1.1 - 0.05).astype(np.float16)
    occ = np.linalg.norm(q.astype(np.float32) - 0.5, axis=1) < 0.3
    os.makedirs(os.path.join(str(tmp_path), "eval", sub), exist_ok=True)
    np.savez(os.path.join(str(tmp_path), "eval", sub, "points.npz"), points=q, occupancies=np.packbits(occ))
    gt = _surface(n_gt, rng)
    np.savez(os.path.join(str(tmp_path), "eval", sub, "pointcloud.npz"), points=gt)
    os.makedirs(os.path.join(str(tmp_path), "gt"), exist_ok=True)
    np.savez(os.path.join(str(tmp_path), "gt", "0_3dt.npz"), **scene)
    return q.astype(np.float32), occ, gt


def _metrics_clf(metrics, solver="gpu"):
    clf = Config(temp=Config(graph_cut=0, fix_orientation=0, metrics=metrics, device=DEV))
    if solver:
        clf.evaluation = Config(solver=solver, seed=0)
    return clf


def _want_metrics(scene, labels, q, occ, gt):
    from dgnn_amd import ops
    from scipy.spatial import Delaunay
    cells = _locate(scene, q)
    pred = (cells >= 0) & (labels[np.maximum(cells, 0)] == 0)
    s = Delaunay(scene["vertices"]).find_simplex(q.astype(np.float64))
    assert (pred != ((s >= 0) & (labels[np.maximum(s, 0)] == 0))).sum() <= 1
    ids = mm.interface_ids(labels, scene["nfacets"])
    recon, _, cum = ops.sample_interface(scene["vertices"], scene["facets"], ids, len(gt), seed=0, return_cum=True)
    want_recon, _ = mm.sample(scene["vertices"], scene["facets"], ids, cum.cpu().numpy(), len(gt), 0)
    assert np.array_equal(recon.cpu().numpy(), want_recon)
    d1, _ = mm.nn_brute(want_recon, gt)
    d2, _ = mm.nn_brute(gt, want_recon)
    return mm.iou(pred, occ), 0.5 * (d1.astype(np.float64).mean() + d2.astype(np.float64).mean()), ids


@pytest.fixture
def current_device_calls(monkeypatch):
    """Records every call of torch.cuda.current_device() made from the package: the metrics must run where their tensors are (the
    project addresses its GPU as cuda:<n> and never calls set_device), so with one GPU a fallback to the current device is still seen."""
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


def test_iou_gpu_runs_on_the_device_of_its_labels(tmp_path, current_device_calls):
    from dgnn_amd.processing.generate_mesh import iou_gpu
    scene = mm.random_scene(2000, seed=8)
    q, occ, _ = _write_eval(tmp_path, scene, n_gt=10)
    labels = mm.sphere_labels(scene)
    data = Config(path=str(tmp_path), id="m", category="", filename="0")
    got = iou_gpu(data, scene, torch.from_numpy(labels).to(DEV))
    cells = _locate(scene, q)
    assert got == mm.iou((cells >= 0) & (labels[np.maximum(cells, 0)] == 0), occ)
    assert current_device_calls == []


def test_generate_fills_iou_and_chamfer_on_the_gpu(tmp_path, capsys, current_device_calls):
    from dgnn_amd.processing.generate_mesh import generate
    rng = np.random.default_rng(3)
    scene = mm.scene_from_points(rng.random((3000, 3)))
    q, occ, gt = _write_eval(tmp_path, scene)
    n = len(scene["tetrahedra"])
    sd = np.linalg.norm(mm.centroids(scene) - 0.5, axis=1) - 0.3
    pred = torch.from_numpy(np.stack([-sd, sd], 1).astype(np.float32))
    data = Config(path=str(tmp_path), gtfile="gt/0", filename="0", id="m", category="", infinite=torch.zeros(n, dtype=torch.int32))
    mesh, ev = generate(data, pred.to(DEV), _metrics_clf(["iou", "chamfer"]))
    assert current_device_calls == []                   # generate's metrics ran where its labels are
    labels = (sd > 0).astype(np.int32)
    want_iou, want_ch, ids = _want_metrics(scene, labels, q, occ, gt)
    assert set(ev) == {"iou", "chamfer"}
    assert ev["iou"] == want_iou and 0.5 < ev["iou"] < 1.0
    assert abs(ev["chamfer"] - want_ch) <= 1e-12 * want_ch
    assert "WARNING" not in capsys.readouterr().out
    # faces unchanged by the key
    mesh0, ev0 = generate(data, pred.to(DEV), _metrics_clf(["iou", "chamfer"], solver=None))
    assert np.array_equal(np.asarray(mesh.faces), np.asarray(mesh0.faces))
    try:
        import trimesh  # noqa: F401
    except ImportError:
        assert ev0 == {} and np.array_equal(np.asarray(mesh.faces), scene["facets"][ids])
    # ioufile wins when set; a failing IoU gives 0.0 with the reference's warning
    data.ioufile = os.path.join("eval", "m", "points.npz")
    _, ev2 = generate(data, pred.to(DEV), _metrics_clf(["iou"]))
    assert ev2 == {"iou": want_iou}
    data.ioufile = ""
    np.savez(os.path.join(str(tmp_path), "eval", "m", "points.npz"), points=np.full((4, 3), np.nan, np.float32), occupancies=np.packbits(np.ones(4, bool)))
    _, ev3 = generate(data, pred.to(DEV), _metrics_clf(["iou"]))
    assert ev3 == {"iou": 0.0} and "WARNING: Could not calculate IoU for mesh" in capsys.readouterr().out


def test_generate_empty_interface_gives_inf(tmp_path, capsys):
    from dgnn_amd.processing.generate_mesh import generate
    scene = mm.random_scene(500, seed=1)
    q, occ, gt = _write_eval(tmp_path, scene, n_gt=300)
    n = len(scene["tetrahedra"])
    data = Config(path=str(tmp_path), gtfile="gt/0", filename="0", id="m", category="", infinite=torch.zeros(n, dtype=torch.int32))
    pred = torch.zeros(n, 2)
    pred[:, 1] = 1.0                                               # every cell outside: no interface
    mesh, ev = generate(data, pred.to(DEV), _metrics_clf(["chamfer", "iou"]))
    assert len(np.asarray(mesh.faces)) == 0
    assert ev["chamfer"] == float("inf") and ev["iou"] == 0.0
    assert "has no faces" in capsys.readouterr().out


@pytest.mark.parametrize("metric", ["iou", "chamfer"])
def test_train_test_validates_on_gpu_mesh_metrics(tmp_path, capsys, metric):
    from dgnn_amd.learning.runModel import Trainer
    from dgnn_amd.sampler import NeighborSampler
    from test_gpu_parity import hip_static
    from test_trainer_cpu import make_clf, small_scene
    clf = make_clf(tmp_path)
    clf.temp.device = DEV
    clf.temp.metrics = [metric]
    clf.temp.graph_cut = 0
    clf.temp.fix_orientation = 0
    clf.evaluation = Config(solver="gpu", seed=0)
    adj, n, x, ea, y = small_scene(600, seed=5)
    pts = np.random.default_rng(5).random((600, 3))                  # the points delaunay_tet_graph(600, seed=5) triangulates
    scene = mm.scene_from_points(pts)
    nf = len(scene["tetrahedra"])
    _write_eval(tmp_path, scene, n_gt=2000)
    infinite = torch.cat([torch.zeros(nf), torch.ones(n - nf)])
    ei = torch.from_numpy(adj.T.astype(np.int64)).to(DEV)
    all_ = Config(x=x.to(DEV), y=y.to(DEV), edge_attr=ea.to(DEV))
    loader = NeighborSampler(ei, sizes=[-1] * 4, node_idx=torch.arange(0, 3 * 64), num_nodes=n, batch_size=64)
    val = Config(x=all_.x, y=all_.y, edge_attr=all_.edge_attr, edge_index=ei, infinite=infinite, path=str(tmp_path), gtfile="gt/0",
                 filename="0", id="m", category="")
    data = Config(train=Config(all=all_, batches=loader), validation=Config(all=[val], batches=[[]]))
    rows = Trainer(hip_static(train=True)).train_test(data, clf)
    assert "Could not calculate" not in capsys.readouterr().out         # the device metric, not the warning's fallback value
    assert "model_best.ptm" in os.listdir(os.path.join(str(tmp_path), "models"))
    vals = [r["test_current_" + metric] for r in rows if "test_current_" + metric in r]
    assert vals and all(np.isfinite(v) or v == float("inf") for v in vals)
    if metric == "iou":
        assert all(0.0 <= v <= 1.0 for v in vals)
