"""scene_from_scan (dgnn_amd/processing/scan_scene.py): a raw scan with outliers -> a folder that dataLoader.run loads under the
reference's shipped feature lists with inference.has_label off, and that the shipped weights run on.  Mirrors the made_scene fixture of
tests/test_gpu_scene_fgeom.py, with the scan in place of the mesh."""
import os

import numpy as np
import pytest
import torch

import knn_model as km
import mesh_contains_model as mc
from helpers import kf96_state_dict, oracle_static
from dgnn_amd.config import Config, reconbench_pretrained

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_LOGIT = 1e-4          # tests/test_gpu_scene_fgeom.py, tests/test_gpu_parity.py: the device's logits against the reference's
NODE_FEATURES = ["shape", "vertex", "facet", "count", "min", "max", "sum", "first", "second"]          # the reference's shipped lists
EDGE_FEATURES = ["shape", "vertex", "facet", "count", "min", "max", "sum"]
FILES = ("_3dt", "_adjacencies", "_cgeom", "_cbvf", "_fbvf", "_cbff", "_fbff", "_fgeom", "_labels")


@pytest.fixture(scope="module")
def scan_scene(tmp_path_factory):
    """a 300-face sphere scanned with a tenth of outliers, the scan alone handed on -> (base, scan, scene, loader, clf)"""
    from dgnn_amd.processing.data import dataLoader
    from dgnn_amd.processing.scan_mesh import scan_mesh
    from dgnn_amd.processing.scan_scene import scene_from_scan
    root = str(tmp_path_factory.mktemp("scan_scene"))
    gv, gf = mc.sphere_interface(300)
    scan = scan_mesh(gv, gf, points=1500, cameras=10, outliers=0.1, seed=1, device=DEV)
    base = os.path.join(root, "gt", "0")
    scene = scene_from_scan(scan["points"], scan["sensor_position"], base, facet_rays=True, facet_geometry=True, scan_file=os.path.join(root, "scan.npz"), device=DEV)
    clf = reconbench_pretrained(device=DEV)
    clf.features.node_features, clf.features.edge_features = list(NODE_FEATURES), list(EDGE_FEATURES)
    clf.temp.cell_order = "none"
    clf.inference.has_label = False
    dl = dataLoader(clf, verbosity=0)
    dl.run(dict(path=root, filename="0", category="", id="", scan_conf="", gtfile="gt/0", ioufile=""))
    dl.getInfo()
    return base, scan, scene, dl, clf


def test_all_nine_files_and_labels_hold_infinite_alone(scan_scene):
    base, scan, scene, dl, clf = scan_scene
    for suffix in FILES:
        assert os.path.exists(base + suffix + ".npz"), suffix
    assert len(os.listdir(os.path.dirname(base))) == len(FILES) == 9
    lab = np.load(base + "_labels.npz")
    assert lab.files == ["infinite"] and np.array_equal(lab["infinite"], scene["triangulation"]["infinite"])
    assert sorted(scene) == ["features", "scan", "triangulation"]
    z = np.load(os.path.join(os.path.dirname(os.path.dirname(base)), "scan.npz"))
    assert z.files == ["points", "normals", "sensor_position"]
    for k in z.files:
        assert z[k].dtype == np.float64 and np.array_equal(z[k], scene["scan"][k]) and z[k].shape == (len(scene["scan"]["kept"]), 3)


def test_the_kept_points_are_the_models_and_no_removed_point_is_a_vertex(scan_scene):
    from dgnn_amd.processing.scene_features import match_vertices
    base, scan, scene, dl, clf = scan_scene
    cleaned = scene["scan"]
    keep, want = km.outlier_mask(scan["points"], k=16, std_ratio=2.0)
    kept = np.nonzero(keep)[0]
    assert cleaned["kept"].dtype == np.int64 and np.array_equal(cleaned["kept"], kept) and cleaned["stats"]["n_removed"] == want["n_removed"] > 0
    for key in ("mu", "sigma", "threshold"):
        assert cleaned["stats"][key] == want[key], key
    assert np.array_equal(cleaned["points"], scan["points"][kept]) and np.array_equal(cleaned["sensor_position"], scan["sensor_position"][kept])
    want_n, _ = km.normals(cleaned["points"], k=16, sensors=cleaned["sensor_position"])
    assert np.array_equal(cleaned["normals"].view(np.int64), want_n.view(np.int64))
    vertices = np.load(base + "_3dt.npz")["vertices"]
    removed = np.setdiff1d(np.arange(len(scan["points"])), kept)
    assert (match_vertices(vertices, scan["points"][removed]) == -1).all() and (match_vertices(vertices, cleaned["points"]) >= 0).all()
    # reported, not asserted: what the default mask does to this scan's injected outliers and to its surface points
    injected = scan["hit_face"] < 0
    cos = np.abs((cleaned["normals"] * scan["gt_normals"][kept]).sum(axis=1))[~injected[kept]]
    print("scan: %d points, %d injected outliers; removed %d: %d of the injected, %d surface points; |cos| of the estimated to the true normal on the kept "
          "surface points: median %.4f, 5th percentile %.4f" % (len(injected), injected.sum(), len(removed), injected[removed].sum(), (~injected[removed]).sum(),
                                                               np.median(cos), np.percentile(cos, 5)))


def test_the_folder_loads_with_has_label_off(scan_scene):
    base, scan, scene, dl, clf = scan_scene
    n = len(scene["triangulation"]["infinite"])
    assert clf.temp.num_node_features == 28 and clf.temp.num_edge_features == 20
    assert dl.features.shape == (n, 29) and dl.edge_features.shape == (4 * n, 20)
    assert tuple(dl.gt.shape) == (n,) and not bool(dl.gt.any()) and int(dl.infinite.sum()) == int(scene["triangulation"]["infinite"].sum())
    assert bool(torch.isfinite(dl.features).all()) and bool(torch.isfinite(dl.edge_features).all())


def test_the_shipped_weights_run_on_a_scene_from_a_scan(scan_scene):
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import SurfaceNet
    base, scan, scene, dl, clf = scan_scene
    net = SurfaceNet(reconbench_pretrained(device=DEV))
    net.load_state_dict(kf96_state_dict())
    net = net.to(DEV).eval()
    ei = dl.edge_lists.contiguous()
    logits = net.inference_layer(Config(x=dl.features, edge_attr=dl.edge_features, edge_index=ei))
    with torch.no_grad():
        ref = oracle_static().inference_layer(Config(x=dl.features.cpu(), edge_attr=dl.edge_features.cpu(), edge_index=ei.cpu()))
    err = (logits.cpu() - ref).abs().max().item()
    print("n = %d cells, max |logit| = %.3g, max |dlogit| = %.3g" % (ref.size(0), ref.abs().max().item(), err))
    assert tuple(logits.shape) == (dl.features.size(0), 2) and bool(torch.isfinite(logits).all())
    assert err <= TOL_LOGIT


def test_without_cleaning_every_distinct_point_is_a_vertex(scan_scene, tmp_path):
    from dgnn_amd.processing.scan_scene import clean_scan, scene_from_scan
    from dgnn_amd.processing.triangulate import drop_duplicates
    base, scan, scene, dl, clf = scan_scene
    raw = scene_from_scan(scan["points"], scan["sensor_position"], str(tmp_path / "raw" / "0"), clean=False, device=DEV)
    distinct = drop_duplicates(scan["points"])[0]
    assert np.array_equal(raw["triangulation"]["mdata"]["vertices"], distinct) and raw["scan"]["normals"] is None and raw["scan"]["stats"] is None
    assert sorted(os.listdir(str(tmp_path / "raw"))) == ["0_3dt.npz", "0_adjacencies.npz", "0_cbvf.npz", "0_cgeom.npz", "0_fbvf.npz", "0_labels.npz"]
    assert len(distinct) > len(scene["triangulation"]["mdata"]["vertices"])
    unmasked = clean_scan(scan["points"], scan["sensor_position"], std_ratio=None, device=DEV)          # normals only
    assert np.array_equal(unmasked["kept"], np.arange(len(scan["points"]))) and unmasked["stats"] is None and unmasked["normals"].shape == scan["points"].shape
