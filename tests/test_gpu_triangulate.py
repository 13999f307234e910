"""The scene layer (dgnn_amd/processing/triangulate.py): a closed mesh becomes, through scan_mesh -> triangulate_scan -> build_scene_features ->
build_cell_labels, a scene folder that dataLoader.run reads.  Counts and ids only: everything asserted is exact."""
import os

import numpy as np
import pytest
import torch

import mesh_contains_model as mc
from dgnn_amd.config import reconbench_pretrained

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_duplicates_are_dropped_on_the_bits():
    from dgnn_amd.processing.triangulate import drop_duplicates, triangulate_scan

    rng = np.random.default_rng(0)
    P = rng.random((60, 3))
    P[5, 1] = 0.0
    Q = np.concatenate([P, P[[7, 5, 7]]])
    Q[61, 1] = -0.0                                        # -0.0 and 0.0 are one value
    verts, kept, dropped = drop_duplicates(Q)
    assert dropped == 3 and np.array_equal(kept, np.arange(60)) and np.array_equal(verts, P)
    tri = triangulate_scan(Q, device=DEV)
    assert tri["n_dropped"] == 3 and len(tri["mdata"]["vertices"]) == 60
    assert len(np.unique(tri["mdata"]["tetrahedra"])) == 60


def test_a_mesh_becomes_a_scene_folder_the_loader_reads(tmp_path):
    from dgnn_amd import ops
    from dgnn_amd.processing.data import dataLoader
    from dgnn_amd.processing.triangulate import make_scene
    from dgnn_amd.synthetic import check_four_regular

    gv, gf = mc.sphere_interface(300)
    base = os.path.join(str(tmp_path), "gt", "0")
    scene = make_scene(gv, gf, base, points=1500, cameras=10, seed=1, device=DEV)
    tri, feat, lab = scene["triangulation"], scene["features"], scene["labels"]
    print(tri["stats"], feat["stats"], lab["stats"])
    for suffix in ("_3dt", "_adjacencies", "_cgeom", "_cbvf", "_fbvf", "_labels"):
        assert os.path.exists(base + suffix + ".npz"), suffix

    # 4. every scan point is a vertex and casts (or shares) a ray; no flat cell; at least one infinite cell per hull facet
    assert feat["stats"]["unmatched_points"] == 0 and feat["stats"]["n_flat"] == 0
    T, N = len(tri["mdata"]["tetrahedra"]), len(tri["infinite"])
    assert N - T == len(tri["hull_facets"]) > 0 and tri["infinite"][:T].sum() == 0 and tri["infinite"][T:].all()

    # 2. the loader reads the folder
    clf = reconbench_pretrained(device=DEV)
    clf.features.node_features = ["shape", "vertex", "count", "min", "max", "sum"]
    clf.features.edge_features = ["vertex", "count", "min", "max", "sum"]
    clf.temp.cell_order = "none"
    dl = dataLoader(clf, verbosity=0)
    dl.run(dict(path=str(tmp_path), filename="0", category="", id="", scan_conf="", gtfile="gt/0", ioufile=""))
    assert dl.features.size(0) == N and dl.edge_features.size(0) == 4 * N and tuple(dl.edge_lists.shape) == (2, 4 * N)
    assert int(dl.infinite.sum()) == N - T and bool(torch.isfinite(dl.features).all()) and bool(torch.isfinite(dl.edge_features).all())

    # 3. the written adjacency: 4-regular over all cells, and its finite part is what ops.tet_neighbors makes of the written _3dt
    m = np.load(base + "_3dt.npz")
    adj = np.load(base + "_adjacencies.npz")["adjacencies"]
    assert adj.dtype == np.int32 and adj.shape == (4 * N, 2) and check_four_regular(adj)
    nbr = ops.tet_neighbors(torch.from_numpy(m["facets"]).to(DEV), torch.from_numpy(m["nfacets"]).to(DEV), torch.from_numpy(m["tetrahedra"]).to(DEV))
    written = adj[:4 * T, 1].reshape(T, 4)
    assert np.array_equal(nbr.cpu().numpy(), np.where(written >= T, -1, written))
    nf = m["nfacets"]
    assert np.all(nf[:, 0] >= 0) and np.all((nf[:, 1] > nf[:, 0]) | (nf[:, 1] == -1)) and np.all(np.diff(nf[:, 0]) >= 0)
    assert len(m["facets"]) == (4 * T + (N - T)) // 2

    # 5. the interface of the labels is a closed surface
    inside = np.load(base + "_labels.npz")["inside_perc"] > 0.5
    assert not inside[T:].any() and inside[:T].any()
    side = np.where(nf >= 0, inside[np.maximum(nf, 0)], False)
    faces = m["facets"][side[:, 0] != side[:, 1]]
    topo = ops.mesh_topology(torch.from_numpy(faces).to(DEV), len(m["vertices"]))
    print(topo)
    assert len(faces) > 0 and topo["boundary_edges"] == 0
