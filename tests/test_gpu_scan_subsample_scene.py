"""subsample_scan and the subsampling keys of scene_from_scan (dgnn_amd/processing/scan_scene.py) on the scan of
tests/test_gpu_scan_scene.py: the kept rows are input rows and the models' selection, a thinned scan still makes a folder that loads with
inference.has_label off and that the shipped weights run on, and without the keys nothing changes."""
import os

import numpy as np
import pytest
import torch

import knn_model as km
import mesh_contains_model as mc
import scan_subsample_model as sm
from helpers import kf96_state_dict, oracle_static
from dgnn_amd.config import Config, reconbench_pretrained

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_LOGIT = 1e-4          # tests/test_gpu_scan_scene.py's bound, the project's own: the device's logits against the reference's
NODE_FEATURES = ["shape", "vertex", "facet", "count", "min", "max", "sum", "first", "second"]          # the reference's shipped lists
EDGE_FEATURES = ["shape", "vertex", "facet", "count", "min", "max", "sum"]
FILES = ("_3dt", "_adjacencies", "_cgeom", "_cbvf", "_fbvf", "_cbff", "_fbff", "_fgeom", "_labels")


@pytest.fixture(scope="module")
def scan():
    """the scan of tests/test_gpu_scan_scene.py: a 300-face sphere, a tenth of outliers -> (scan, the longest extent)"""
    from dgnn_amd.processing.scan_mesh import scan_mesh
    gv, gf = mc.sphere_interface(300)
    s = scan_mesh(gv, gf, points=1500, cameras=10, outliers=0.1, seed=1, device=DEV)
    p = s["points"]
    return s, float((p.max(axis=0) - p.min(axis=0)).max())


def _assert_selection(out, scan, n_in):
    kept = out["kept"]
    assert kept.dtype == np.int64 and (np.diff(kept) > 0).all() and (len(kept) == 0 or (0 <= kept[0] and kept[-1] < n_in))          # ascending, unique
    for key in ("points", "sensor_position"):
        assert out[key].dtype == np.float64 and np.array_equal(out[key].view(np.int64), np.ascontiguousarray(scan[key][kept]).view(np.int64)), key
    assert out["stats"]["n_in"] == n_in and out["stats"]["n_out"] == len(kept)


def test_subsample_scan_keeps_the_models_rows(scan):
    from dgnn_amd.processing.scan_scene import subsample_scan
    s, ext = scan
    p, n = s["points"], len(s["points"])
    h, r = ext / 16.0, ext / 20.0
    vox = sm.voxel_subsample(p, h)
    for rep in ("nearest", "first"):
        out = subsample_scan(p, s["sensor_position"], voxel_size=h, representative=rep, device=DEV)
        _assert_selection(out, s, n)
        assert np.array_equal(out["kept"], np.sort(vox[rep])) and out["stats"]["voxels"] == vox["m"] == len(out["kept"]) < n
    for seed in (0, 1):
        out = subsample_scan(p, s["sensor_position"], min_distance=r, seed=seed, device=DEV)
        _assert_selection(out, s, n)
        assert np.array_equal(out["kept"], np.flatnonzero(sm.min_distance_thin(p, r, seed=seed)[0]))
        d2 = km.d2_matrix(out["points"], out["points"])
        np.fill_diagonal(d2, np.inf)
        assert (d2 >= np.float64(r) * np.float64(r)).all() and out["stats"]["thinning"]["n_kept"] == len(out["kept"]) < n
    out = subsample_scan(p, s["sensor_position"], voxel_size=h, min_distance=r, seed=1, device=DEV)
    _assert_selection(out, s, n)
    left = np.sort(vox["nearest"])
    assert np.array_equal(out["kept"], left[sm.min_distance_thin(p[left], r, seed=1)[0]])          # the thinning counts rows among what is left
    d2 = km.d2_matrix(out["points"], out["points"])
    np.fill_diagonal(d2, np.inf)
    assert (d2 >= np.float64(r) * np.float64(r)).all() and 0 < len(out["kept"]) < vox["m"]
    same = subsample_scan(p, s["sensor_position"], device=DEV)          # no step: the scan as it is
    _assert_selection(same, s, n)
    assert len(same["kept"]) == n and sorted(same["stats"]) == ["n_in", "n_out"]
    with pytest.raises(ValueError, match="representative"):
        subsample_scan(p, s["sensor_position"], voxel_size=h, representative="centroid", device=DEV)
    with pytest.raises(ValueError, match="sensor positions"):
        subsample_scan(p, s["sensor_position"][:-1], voxel_size=h, device=DEV)


@pytest.fixture(scope="module")
def thinned_scene(scan, tmp_path_factory):
    from dgnn_amd.processing.data import dataLoader
    from dgnn_amd.processing.scan_scene import scene_from_scan
    s, ext = scan
    root = str(tmp_path_factory.mktemp("thinned_scene"))
    base = os.path.join(root, "gt", "0")
    scene = scene_from_scan(s["points"], s["sensor_position"], base, facet_rays=True, facet_geometry=True, device=DEV, voxel_size=ext / 16.0)
    clf = reconbench_pretrained(device=DEV)
    clf.features.node_features, clf.features.edge_features = list(NODE_FEATURES), list(EDGE_FEATURES)
    clf.temp.cell_order = "none"
    clf.inference.has_label = False
    dl = dataLoader(clf, verbosity=0)
    dl.run(dict(path=root, filename="0", category="", id="", scan_conf="", gtfile="gt/0", ioufile=""))
    dl.getInfo()
    return base, scene, dl, clf


def test_a_voxel_thinned_scene_has_the_same_files_and_its_kept_rows_are_input_rows(scan, thinned_scene):
    from dgnn_amd.processing.scan_scene import clean_scan, subsample_scan
    s, ext = scan
    base, scene, dl, clf = thinned_scene
    assert sorted(os.listdir(os.path.dirname(base))) == sorted("0" + suffix + ".npz" for suffix in FILES)
    cleaned = scene["scan"]
    kept = cleaned["kept"]
    assert kept.dtype == np.int64 and (np.diff(kept) > 0).all() and 0 < len(kept) < len(s["points"])
    assert np.array_equal(cleaned["points"], s["points"][kept]) and np.array_equal(cleaned["sensor_position"], s["sensor_position"][kept])
    sub = subsample_scan(s["points"], s["sensor_position"], voxel_size=ext / 16.0, device=DEV)          # the two steps by hand
    by_hand = clean_scan(sub["points"], sub["sensor_position"], device=DEV)
    assert np.array_equal(kept, sub["kept"][by_hand["kept"]]) and cleaned["subsample"] == sub["stats"]
    assert np.array_equal(cleaned["normals"].view(np.int64), by_hand["normals"].view(np.int64))
    lab = np.load(base + "_labels.npz")
    assert lab.files == ["infinite"] and np.array_equal(lab["infinite"], scene["triangulation"]["infinite"])


def test_a_voxel_thinned_scene_loads_and_the_shipped_weights_run_on_it(thinned_scene):
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import SurfaceNet
    base, scene, dl, clf = thinned_scene
    n = len(scene["triangulation"]["infinite"])
    assert clf.temp.num_node_features == 28 and clf.temp.num_edge_features == 20
    assert dl.features.shape == (n, 29) and dl.edge_features.shape == (4 * n, 20)
    assert tuple(dl.gt.shape) == (n,) and not bool(dl.gt.any()) and int(dl.infinite.sum()) == int(scene["triangulation"]["infinite"].sum())
    assert bool(torch.isfinite(dl.features).all()) and bool(torch.isfinite(dl.edge_features).all())
    net = SurfaceNet(reconbench_pretrained(device=DEV))
    net.load_state_dict(kf96_state_dict())
    net = net.to(DEV).eval()
    ei = dl.edge_lists.contiguous()
    logits = net.inference_layer(Config(x=dl.features, edge_attr=dl.edge_features, edge_index=ei))
    with torch.no_grad():
        ref = oracle_static().inference_layer(Config(x=dl.features.cpu(), edge_attr=dl.edge_features.cpu(), edge_index=ei.cpu()))
    err = (logits.cpu() - ref).abs().max().item()
    print("voxel-thinned scene: %d of %d points, n = %d cells, max |logit| = %.3g, max |dlogit| = %.3g"
          % (len(scene["scan"]["kept"]), scene["scan"]["subsample"]["n_in"], ref.size(0), ref.abs().max().item(), err))
    assert tuple(logits.shape) == (n, 2) and bool(torch.isfinite(logits).all())
    assert err <= TOL_LOGIT


def test_without_the_keys_nothing_changes(scan, tmp_path):
    from dgnn_amd.processing.scan_scene import scene_from_scan
    s, ext = scan
    plain = scene_from_scan(s["points"], s["sensor_position"], str(tmp_path / "a" / "0"), device=DEV)
    keyed = scene_from_scan(s["points"], s["sensor_position"], str(tmp_path / "b" / "0"), device=DEV, voxel_size=None, min_distance=None, seed=5)
    assert sorted(plain["scan"]) == sorted(keyed["scan"]) == ["kept", "normals", "points", "sensor_position", "stats"]
    for key in ("kept", "normals", "points", "sensor_position"):
        assert plain["scan"][key].tobytes() == keyed["scan"][key].tobytes(), key
    assert sorted(os.listdir(str(tmp_path / "a"))) == sorted(os.listdir(str(tmp_path / "b")))
    for name in sorted(os.listdir(str(tmp_path / "a"))):
        za, zb = np.load(str(tmp_path / "a" / name)), np.load(str(tmp_path / "b" / name))
        assert za.files == zb.files
        for key in za.files:
            assert za[key].dtype == zb[key].dtype and za[key].tobytes() == zb[key].tobytes(), (name, key)
