"""The facet-ray files of a scene (build_scene_features(facet_rays=True), make_scene(facet_rays=True), processing.visibility):
layout as in the golden small scene's `_cbff` / `_fbff`, values equal to the model's walk (tests/ray_walk_model.py) bit for bit, infinite rows 0,
nothing changed without the flag, the files load through dataLoader.run with `facet` in both feature lists, and the visibility votes with the
graph cut label every infinite cell outside."""
import functools
import os

import numpy as np
import pytest
import torch

import mesh_contains_model as mc
import mesh_metrics_model as mm
import ray_walk_model as rw
import scene_features_model as sf
from helpers import gold
from dgnn_amd.config import reconbench_pretrained

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


@functools.lru_cache(maxsize=None)
def _built(out_base=None, facet_rays=True):
    from dgnn_amd.processing.scene_features import build_scene_features
    scan, mdata, infinite = _scanned_cube()
    return build_scene_features(mdata, infinite, scan["points"], scan["sensor_position"], out_base=out_base, device=DEV, facet_rays=facet_rays)


@functools.lru_cache(maxsize=None)
def _model():
    scan, mdata, infinite = _scanned_cube()
    nbr, bad = sf.tet_neighbors(mdata["facets"], mdata["nfacets"], mdata["tetrahedra"])
    assert bad == 0
    vid = sf.match_vertices(mdata["vertices"], scan["points"])
    assert (vid >= 0).all()
    return rw.ray_walk(mdata["vertices"], mdata["tetrahedra"], nbr, vid, scan["sensor_position"])          # the defaults: depths 0 and 1


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def test_layout_is_the_golden_files_and_values_are_the_models():
    out, want = _built(), _model()
    scan, mdata, infinite = _scanned_cube()
    n, t = len(infinite), len(mdata["tetrahedra"])
    assert out["walk_stats"] == {k: want["stats"][k] for k in out["walk_stats"]}
    print(out["walk_stats"])
    assert want["stats"]["records"] > 300 and want["stats"]["stuck"] == 0 and want["stats"]["capped"] == 0 and want["stats"]["depth"] > 100
    for name, rows in (("cbff", n), ("fbff", 4 * n)):
        g = gold("scene_small/gt/0_%s.npz" % name)
        assert list(out[name]) == list(g.files), name
        for k in g.files:
            assert out[name][k].dtype == g[k].dtype == np.float64 and out[name][k].shape == (rows,) and g[k].ndim == 1, k
            if "_last_" in k:
                assert not out[name][k].any(), k
    for side in rw.SIDES:
        for which in ("first", "second"):
            for stat, key in (("count", "cell_count"), ("dist_min", "cell_%s_min" % which), ("dist_max", "cell_%s_max" % which), ("dist_sum", "cell_%s_sum" % which)):
                col = out["cbff"]["cb_facet_%s_%s_%s" % (side, which, stat)]
                assert np.array_equal(_bits(col[:t]), _bits(want["%s_%s" % (side, key)].astype(np.float64))) and not col[t:].any(), (side, which, stat)
        for stat in ("count", "min", "max", "sum"):
            col = out["fbff"]["fb_facet_%s_%s" % (side, stat if stat == "count" else "dist_" + stat)]
            assert np.array_equal(_bits(col[:4 * t]), _bits(want["%s_slot_%s" % (side, stat)].astype(np.float64).reshape(-1))) and not col[4 * t:].any()
    assert out["cbff"]["cb_facet_inside_first_count"].sum() == want["ray_cells"][:, 1].sum() and out["cbff"]["cb_facet_outside_first_count"].sum() > 0


def test_without_the_flag_the_result_and_the_files_are_todays(tmp_path):
    from dgnn_amd.processing.scene_features import build_scene_features
    scan, mdata, infinite = _scanned_cube()
    plain = build_scene_features(mdata, infinite, scan["points"], scan["sensor_position"], out_base=str(tmp_path / "0"), device=DEV)
    assert sorted(plain) == ["cbvf", "cgeom", "fbvf", "mean_edge", "neighbors", "stats"]
    assert sorted(os.listdir(str(tmp_path))) == ["0_cbvf.npz", "0_cgeom.npz", "0_fbvf.npz"]
    full = _built()
    assert sorted(set(full) - set(plain)) == ["cbff", "fbff", "walk_stats"] and full["stats"] == plain["stats"]
    for name in ("cgeom", "cbvf", "fbvf"):
        assert list(full[name]) == list(plain[name]) and all(np.array_equal(_bits(full[name][k]), _bits(plain[name][k])) for k in plain[name]), name


def _facet_config():
    """reconbench_pretrained with `facet` in both feature lists (a copy: tests/configs stays as it is)"""
    clf = reconbench_pretrained(device=DEV)
    clf.features.node_features = ["shape", "vertex", "facet", "count", "min", "max", "sum"]
    clf.features.edge_features = ["vertex", "facet", "count", "min", "max", "sum"]
    clf.temp.cell_order = "none"
    return clf


def test_make_scene_chains_to_a_folder_the_loader_reads_with_the_facet_features(tmp_path):
    from dgnn_amd.processing.data import dataLoader
    from dgnn_amd.processing.triangulate import make_scene
    gv, gf = mc.sphere_interface(300)
    base = os.path.join(str(tmp_path), "gt", "0")
    scene = make_scene(gv, gf, base, points=1500, cameras=10, seed=1, device=DEV, facet_rays=True)
    feat, tri = scene["features"], scene["triangulation"]
    print(feat["walk_stats"])
    for suffix in ("_3dt", "_adjacencies", "_cgeom", "_cbvf", "_fbvf", "_cbff", "_fbff", "_labels"):
        assert os.path.exists(base + suffix + ".npz"), suffix
    n, t = len(tri["infinite"]), len(tri["mdata"]["tetrahedra"])
    z = np.load(base + "_cbff.npz")
    assert z.files == gold("scene_small/gt/0_cbff.npz").files and np.load(base + "_fbff.npz").files == gold("scene_small/gt/0_fbff.npz").files
    assert all(np.array_equal(_bits(z[k]), _bits(feat["cbff"][k])) for k in z.files)
    ws = feat["walk_stats"]
    assert ws["stuck"] == 0 and ws["capped"] == 0 and ws["used"] == feat["stats"]["used"] and ws["records"] > ws["used"]
    assert z["cb_facet_outside_first_count"][:t].sum() > 0 and not z["cb_facet_outside_first_count"][t:].any()
    dl = dataLoader(_facet_config(), verbosity=0)
    dl.run(dict(path=str(tmp_path), filename="0", category="", id="", scan_conf="", gtfile="gt/0", ioufile=""))
    # the regularisation column, shape, vertex, facet; the `last` groups are dropped
    assert dl.features.shape == (n, 1 + 4 + 8 + 16) and dl.edge_features.shape == (4 * n, 8 + 8)
    assert sum("cb_facet" in k for k in dl.node_feature_names) == 16 and sum("fb_facet" in k for k in dl.edge_feature_names) == 8
    assert bool(torch.isfinite(dl.features).all()) and bool(torch.isfinite(dl.edge_features).all())


def test_visibility_votes_are_their_formula_and_the_graph_cut_puts_every_infinite_cell_outside():
    from dgnn_amd import ops
    from dgnn_amd.processing.visibility import visibility_logits
    out = _built()
    scan, mdata, infinite = _scanned_cube()
    n, t = len(infinite), len(mdata["tetrahedra"])
    votes = visibility_logits(out, infinite, 7.5)
    assert votes.dtype == torch.float32 and tuple(votes.shape) == (n, 2)
    inf = infinite.astype(bool)
    for j, side in enumerate(("inside", "outside")):
        want = (out["cbvf"]["cb_vertex_%s_count" % side] + out["cbff"]["cb_facet_%s_first_count" % side]).astype(np.float32)
        assert np.array_equal(votes[:, j].numpy()[~inf], want[~inf])
    assert (votes[inf].numpy() == [0.0, 7.5]).all() and votes[:, 0].sum() > 0 and votes[:, 1].sum() > 0
    nb = out["neighbors"]
    c, k = np.nonzero(nb > np.arange(n)[:, None])          # every finite-finite facet once
    hull = np.nonzero((nb[:t] < 0).reshape(-1))[0] // 4          # the finite cell of every hull facet, in the order of the infinite cells' count
    assert len(hull) == n - t
    edges = np.concatenate([np.stack([c, nb[c, k]], axis=1), np.stack([hull, t + np.arange(n - t)], axis=1)])
    labels, _, _ = ops.binary_graph_cut(votes, edges, 1.0, 1.0)
    labels = labels.cpu().numpy()
    assert (labels[inf] == 1).all() and (labels[~inf] == 0).any()
    with pytest.raises(ValueError):
        visibility_logits(out, infinite[:-1], 1.0)
