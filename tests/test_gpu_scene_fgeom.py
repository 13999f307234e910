"""`<scene>_fgeom.npz`, the last file of a made scene (build_scene_features(facet_geometry=True), make_scene(facet_geometry=True)):
its layout and values, nothing changed beside it, and the chain it closes -- a scene made from a mesh loads under the reference's shipped
feature lists, unedited, and the shipped weights run on it."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_contains_model as mc
import mesh_metrics_model as mm
from helpers import kf96_state_dict, oracle_static
from dgnn_amd.config import Config, reconbench_pretrained

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_LOGIT = 1e-4          # tests/test_gpu_parity.py: the device's logits against the reference's on the Ignatius block
NODE_FEATURES = ["shape", "vertex", "facet", "count", "min", "max", "sum", "first", "second"]          # the reference's shipped lists
EDGE_FEATURES = ["shape", "vertex", "facet", "count", "min", "max", "sum"]
FILES = ("_3dt", "_adjacencies", "_cgeom", "_cbvf", "_fbvf", "_cbff", "_fbff", "_fgeom", "_labels")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _scanned_cube():
    """a noisy scan of a cube, scipy's cells of its points, one infinite cell per hull facet -> (scan, mdata, infinite); read only"""
    from dgnn_amd.processing.scan_mesh import scan_mesh
    from dgnn_amd.processing.triangulate import drop_duplicates
    scan = scan_mesh(*mc.cube(0.2, 0.8), points=400, cameras=6, noise=0.01, seed=2, device=DEV)
    mdata = mm.scene_from_points(drop_duplicates(scan["points"])[0])
    n_hull = int((mdata["nfacets"][:, 1] < 0).sum())
    infinite = np.concatenate([np.zeros(len(mdata["tetrahedra"]), np.int32), np.ones(n_hull, np.int32)])
    return scan, mdata, infinite


def test_the_flag_adds_the_file_and_changes_nothing_else(tmp_path):
    from dgnn_amd import ops
    from dgnn_amd.processing.scene_features import FGEOM_KEYS, build_scene_features
    scan, mdata, infinite = _scanned_cube()
    n, t = len(infinite), len(mdata["tetrahedra"])
    plain = build_scene_features(mdata, infinite, scan["points"], scan["sensor_position"], device=DEV)
    full = build_scene_features(mdata, infinite, scan["points"], scan["sensor_position"], out_base=str(tmp_path / "0"), device=DEV, facet_geometry=True)
    assert sorted(set(full) - set(plain)) == ["fgeom", "fgeom_stats"] and full["stats"] == plain["stats"]
    for name in ("cgeom", "cbvf", "fbvf"):
        assert list(full[name]) == list(plain[name]) and all(np.array_equal(_bits(full[name][k]), _bits(plain[name][k])) for k in plain[name]), name
    assert sorted(os.listdir(str(tmp_path))) == ["0_cbvf.npz", "0_cgeom.npz", "0_fbvf.npz", "0_fgeom.npz"]
    z = np.load(str(tmp_path / "0_fgeom.npz"))
    assert tuple(z.files) == tuple(FGEOM_KEYS) == ("area", "cos_own", "cos_neighbor", "beta")
    op = ops.facet_geometry(mdata["vertices"], mdata["tetrahedra"], mdata["facets"], mdata["nfacets"])
    assert full["fgeom_stats"] == op["stats"] and op["stats"]["rows"] == 4 * t and op["stats"]["hull_rows"] == n - t
    for k in FGEOM_KEYS:
        assert z[k].dtype == np.float64 and z[k].shape == (4 * n,) and np.array_equal(_bits(z[k]), _bits(full["fgeom"][k])), k
        assert not z[k][4 * t:].any(), k                                                          # the rows of the infinite cells
        assert np.array_equal(_bits(z[k][:4 * t]), _bits(op[k].cpu().numpy())) and np.isfinite(z[k]).all(), k
    assert (z["area"][:4 * t] > 0).all() and (z["cos_neighbor"][:4 * t] == 1.0).sum() >= n - t


def test_a_triangulation_that_misses_a_facet_is_refused(tmp_path):
    from dgnn_amd.processing.scene_features import build_scene_features
    scan, mdata, infinite = _scanned_cube()
    inner = int(np.nonzero((mdata["nfacets"] >= 0).all(axis=1))[0][0])
    short = dict(mdata, facets=np.delete(mdata["facets"], inner, axis=0), nfacets=np.delete(mdata["nfacets"], inner, axis=0))
    with pytest.raises(ValueError, match="every facet"):
        build_scene_features(short, infinite, scan["points"], scan["sensor_position"], out_base=str(tmp_path / "0"), device=DEV, facet_geometry=True)
    assert not os.path.exists(str(tmp_path / "0_fgeom.npz"))


@pytest.fixture(scope="module")
def made_scene(tmp_path_factory):
    """the sphere scene of tests/test_gpu_facet_features.py with both flags, loaded under the shipped lists -> (base, scene, loader, clf)"""
    from dgnn_amd.processing.data import dataLoader
    from dgnn_amd.processing.triangulate import make_scene
    root = str(tmp_path_factory.mktemp("fgeom_scene"))
    gv, gf = mc.sphere_interface(300)
    base = os.path.join(root, "gt", "0")
    scene = make_scene(gv, gf, base, points=1500, cameras=10, seed=1, device=DEV, facet_rays=True, facet_geometry=True)
    clf = reconbench_pretrained(device=DEV)
    clf.features.node_features, clf.features.edge_features = list(NODE_FEATURES), list(EDGE_FEATURES)
    clf.temp.cell_order = "none"
    dl = dataLoader(clf, verbosity=0)
    dl.run(dict(path=root, filename="0", category="", id="", scan_conf="", gtfile="gt/0", ioufile=""))
    dl.getInfo()
    return base, scene, dl, clf


def test_a_made_scene_loads_under_the_shipped_feature_lists(made_scene):
    from dgnn_amd.processing.scene_features import FGEOM_KEYS
    base, scene, dl, clf = made_scene
    for suffix in FILES:
        assert os.path.exists(base + suffix + ".npz"), suffix
    assert len(os.listdir(os.path.dirname(base))) == len(FILES) == 9
    n = len(scene["triangulation"]["infinite"])
    assert clf.temp.num_node_features == 28 and clf.temp.num_edge_features == 20
    assert dl.features.shape == (n, 29) and dl.edge_features.shape == (4 * n, 20)
    names = [k for k in dl.edge_feature_names if not k.startswith("reg_")]
    assert tuple(names[:4]) == tuple(FGEOM_KEYS) and len(names) == 20
    assert bool(torch.isfinite(dl.features).all()) and bool(torch.isfinite(dl.edge_features).all())
    st = scene["features"]["fgeom_stats"]
    t = len(scene["triangulation"]["mdata"]["tetrahedra"])
    assert st["rows"] == 4 * t and st["hull_rows"] == n - t


def test_the_shipped_weights_run_on_a_made_scene(made_scene):
    """mesh -> scan -> triangulation -> all eight feature files -> shipped config -> shipped weights -> logits, on this stack alone; the logits
    against the oracle's on the same tensors, within the bound of tests/test_gpu_parity.py's comparison on the Ignatius block"""
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import SurfaceNet
    base, scene, dl, clf = made_scene
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
