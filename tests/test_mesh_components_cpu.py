"""The CPU model of the mesh components (tests/mesh_components_model.py) against hand-built answers and against networkx."""
import math

import numpy as np
import pytest

import mesh_components_model as mc
import mesh_metrics_model as mm
from helpers import gold


def _networkx_components(faces):
    """components by an independent route: a bipartite faces / undirected-edges graph"""
    import networkx as nx

    g = nx.Graph()
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    for t, (a, b, c) in enumerate(f):
        g.add_node(("f", t))
        for u, w in ((a, b), (b, c), (c, a)):
            g.add_edge(("f", t), ("e", min(u, w), max(u, w)))
    lab = np.empty(len(f), dtype=np.int64)
    for k, nodes in enumerate(nx.connected_components(g)):
        for node in nodes:
            if node[0] == "f":
                lab[node[1]] = k
    return mc.renumber(lab)


@pytest.mark.parametrize("case", mc.HAND_MADE)
def test_hand_made_meshes_have_the_known_number_of_components(case):
    _, f, k = mc.hand_made(case)
    comp, got = mc.components(f)
    assert got == k and len(comp) == len(f)
    want = {"empty": [], "one_face": [0], "shared_edge": [0, 0], "shared_vertex": [0, 1], "two_tets": [0] * 4 + [1] * 4, "glued_edge": [0] * 8}[case]
    assert comp.tolist() == want


def test_numbering_follows_the_smallest_face_id():
    comp, k = mc.renumber(np.array([7, 3, 7, 5, 3, 9]))
    assert comp.tolist() == [0, 1, 0, 2, 1, 3] and k == 4
    v, f = mc.many_tets(5)
    comp, k = mc.components(f)
    assert k == 5 and comp.tolist() == list(range(5)) * 4          # interleaved: face j * n + t belongs to tetrahedron t
    v, f = mc.shells_and_crumbs()
    comp, k = mc.components(f)
    assert k == 5 and comp.tolist() == [0, 1, 0, 2, 0, 3, 2, 2, 0, 4, 2]


@pytest.mark.parametrize("which", ["strip", "many_tets", "shells", "crumbs_then_strip", "gold", "random_10pct"])
def test_components_equal_networkx(which):
    if which == "strip":
        f = mc.strip(4099, seed=1)[1]
    elif which == "many_tets":
        f = mc.many_tets(200)[1]
    elif which == "shells":
        f = mc.shells_and_crumbs()[1]
    elif which == "crumbs_then_strip":
        f = mc.crumbs_then_strip()[1]
    elif which == "gold":
        f = gold("genmesh_f4_small.npz")["faces"]
    else:
        scene = mm.random_scene(600, seed=3)
        labels = (np.random.default_rng(5).random(len(scene["tetrahedra"])) > 0.1).astype(np.int32)
        f = scene["facets"][mm.interface_ids(labels, scene["nfacets"])]
    comp, k = mc.components(f)
    want, want_k = _networkx_components(f)
    assert k == want_k and np.array_equal(comp, want)
    if which == "strip":
        assert k == 1
    if which == "random_10pct":
        assert k > 3


def test_measures_of_known_solids():
    v, f = mc.unit_tet()
    m = mc.measures(v, f, np.zeros(4, dtype=np.int32), 1)
    assert m["n_faces"].tolist() == [4] and m["signed_volume"][0] == 1.0 / 6.0
    assert abs(m["area"][0] - (1.5 + math.sqrt(3.0) / 2.0)) <= 4 * mc.U * 3
    v, f = mc.unit_tet(flip=True)
    assert mc.measures(v, f, np.zeros(4, dtype=np.int32), 1)["signed_volume"][0] == -1.0 / 6.0
    # the bound is the stated multiple of the absolute sum
    v, f = mc.many_tets(3)
    comp, k = mc.components(f)
    m = mc.measures(v, f, comp, k)
    ta, tv = mc.face_terms(v, f)
    for c in range(k):
        assert m["area_bound"][c] == 7 * mc.U * math.fsum(ta[comp == c]) and m["volume_bound"][c] == 7 * mc.U * math.fsum(np.abs(tv[comp == c]))
        assert m["area"][c] > 0 and abs(m["signed_volume"][c]) > 0
    assert (m["n_faces"] == 4).all()


def test_keep_rules():
    v, f = mc.shells_and_crumbs()
    comp, k = mc.components(f)
    counts = mc.measures(v, f, comp, k)["n_faces"]
    assert counts.tolist() == [4, 1, 4, 1, 1]
    kept, keep, n = mc.filter_faces(f, comp, counts, largest=True)               # a tie of 4 and 4: the smaller id
    assert n == 4 and np.array_equal(np.nonzero(keep)[0], [0, 2, 4, 8]) and np.array_equal(kept, f[[0, 2, 4, 8]])
    kept, keep, n = mc.filter_faces(f, comp, counts, min_faces=4)
    assert n == 8 and np.array_equal(kept, f[[0, 2, 3, 4, 6, 7, 8, 10]]) and set(np.unique(kept)) == {0, 1, 2, 3, 10, 11, 12, 13}
    assert mc.filter_faces(f, comp, counts, min_faces=1)[2] == 11 and mc.filter_faces(f, comp, counts, min_faces=5)[2] == 0
    assert mc.keep_mask(np.zeros(0), np.zeros(0), largest=True).shape == (0,)
