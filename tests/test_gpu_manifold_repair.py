"""ops.vertex_components / ops.manifold_repair (csrc/manifold.hip) against the CPU model tests/manifold_repair_model.py, which
keeps explicit star lists and searches them breadth-first: every element and every stat, on triangulations from ops.delaunay.  The
repaired labels are then handed to the existing kernels (orient_interface, mesh_topology): no singular vertex <=> watertight."""
import numpy as np
import pytest
import torch

import manifold_repair_model as m

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CACHE = {}
CLEAN = [name for name, (_, _, clean) in m.SCENES.items() if clean]


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _triangulate(points):
    from dgnn_amd import ops

    d = ops.delaunay(_t(points))
    tets = d["tetrahedra"].cpu().numpy()
    nbr = d["neighbors"][:len(tets)].cpu().numpy().copy()
    nbr[nbr >= len(tets)] = -1
    return tets, nbr


def _scene(name):
    """(points, tets, nbr, labels) of a model scene on the device's own triangulation; computed once"""
    if name not in _CACHE:
        points, labels, _ = m.SCENES[name]
        pts = points()
        tets, nbr = _triangulate(pts)
        _CACHE[name] = (pts, tets, nbr, labels(pts, tets))
    return _CACHE[name]


def _cost(mode, n):
    return None if mode == "count" else m.margin_cost(n)


def _want(name, mode):
    """the model's repair of a scene, computed once and never written to"""
    key = (name, mode, "want")
    if key not in _CACHE:
        pts, tets, nbr, labels = _scene(name)
        _CACHE[key] = m.repair(tets, nbr, labels, len(pts), cost=_cost(mode, len(tets)))
    return _CACHE[key]


def _repair(tets, nbr, labels, nv, **kw):
    from dgnn_amd import ops

    cost = kw.pop("cost", None)
    return ops.manifold_repair(_t(tets), _t(nbr), _t(labels), nv, cost=None if cost is None else _t(cost), **kw)


def _stats_equal(got, want):
    assert {k: got[k] for k in m.STAT_KEYS} == {k: want[k] for k in m.STAT_KEYS}


def _topology(points, tets, nbr, labels):
    """mesh_topology of the interface the existing kernels extract from `labels` (None: no interface facet)"""
    from dgnn_amd import ops
    from dgnn_amd.processing.generate_mesh import interface_from_labels

    facets, nfacets = m.facets_of(tets, nbr)
    lab = _t(labels)
    ids = interface_from_labels(lab, _t(nfacets))
    if ids.numel() == 0:
        return None
    faces, _ = ops.orient_interface(_t(points), _t(tets), _t(facets), _t(nfacets), lab, ids)
    return ops.mesh_topology(faces, len(points))


@pytest.mark.parametrize("name", list(m.SCENES))
def test_vertex_components_equal_the_model(name):
    from dgnn_amd import ops

    pts, tets, nbr, labels = _scene(name)
    a, b, n_singular = ops.vertex_components(_t(tets), _t(nbr), _t(labels), len(pts))
    want_a, want_b, want_n = m.vertex_components(tets, nbr, labels, len(pts))
    assert np.array_equal(a.cpu().numpy(), want_a) and np.array_equal(b.cpu().numpy(), want_b) and n_singular == want_n
    assert want_n > 0                                                   # every scene has something to repair
    if name == "sphere_centre":                                         # the star-size case: one row holds every cell, far beyond a wavefront
        assert (tets == len(pts) - 1).any(axis=1).all() and len(tets) > 256


@pytest.mark.parametrize("mode", ["count", "margin"])
@pytest.mark.parametrize("name", list(m.SCENES))
def test_repair_equals_the_model(name, mode):
    pts, tets, nbr, labels = _scene(name)
    nv, cost = len(pts), _cost(mode, len(tets))
    want, want_st, want_flipped, history = _want(name, mode)
    got, st, flipped = _repair(tets, nbr, labels, nv, cost=cost, return_flipped=True)
    print(name, mode, st)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(flipped.cpu().numpy(), want_flipped)
    _stats_equal(st, want_st)
    if name in CLEAN:                                                   # a condition: the model reaches it on the CPU, so must the device
        assert want_st["singular_after"] == 0 and st["singular_after"] == 0
    if name == "u300_n50":
        assert st["singular_after"] > 0                                 # stuck vertices: the same ones, reported
        from dgnn_amd import ops
        a, b, _ = ops.vertex_components(_t(tets), _t(nbr), got, nv)
        wa, wb, _ = m.vertex_components(tets, nbr, want, nv)
        assert np.array_equal(a.cpu().numpy(), wa) and np.array_equal(b.cpu().numpy(), wb)
    again, st2 = _repair(tets, nbr, labels, nv, cost=cost)              # reruns are bit-identical
    assert torch.equal(again, got) and st2 == st
    # the tie rule is the cell id, not the corner: the columns of every row permuted (neighbours alike) change nothing
    perm = np.argsort(np.random.default_rng(11).random((len(tets), 4)), axis=1)
    shuffled, st3 = _repair(np.take_along_axis(tets, perm, axis=1), np.take_along_axis(nbr, perm, axis=1), labels, nv, cost=cost)
    assert torch.equal(shuffled, got) and st3 == st
    # the existing kernels agree with the criterion
    topo = _topology(pts, tets, nbr, want)
    if st["singular_after"] == 0:
        assert topo["watertight"] == 1
    else:
        assert topo["nonmanifold_edges"] + topo["nonmanifold_vertices"] > 0 and topo["boundary_edges"] == 0


@pytest.mark.parametrize("name", ["u60_n30", "u800_n5", "sphere_centre"])
def test_max_rounds_only_stops_early(name):
    pts, tets, nbr, labels = _scene(name)
    _, full, _, history = _want(name, "count")
    assert len(history) >= 3
    for r in (1, 2, 3):
        got, st = _repair(tets, nbr, labels, len(pts), max_rounds=r)
        _, want_st, _, _ = m.repair(tets, nbr, labels, len(pts), max_rounds=r)
        assert np.array_equal(got.cpu().numpy(), history[r - 1])
        _stats_equal(st, want_st)
    got, st = _repair(tets, nbr, labels, len(pts), max_rounds=0)       # no round: the labels as given, both counts the first detection's
    assert np.array_equal(got.cpu().numpy(), labels) and st["rounds"] == 0 and st["singular_after"] == st["singular_before"] == full["singular_before"]


HAND = ["edge_pair", "edge_pair_cost", "vertex_pair", "hull_inside", "all_inside", "all_outside", "pocket", "larger_cheaper", "larger_dearer"]


@pytest.mark.parametrize("name", HAND)
def test_hand_built_cases(name):
    from dgnn_amd import ops

    if "hand" not in _CACHE:
        pts = m.uniform_points(60, 7)
        tets, nbr = _triangulate(pts)
        _CACHE["hand"] = (pts, tets, nbr, m.hand_cases(tets, nbr))
    pts, tets, nbr, cases = _CACHE["hand"]
    case, nv = cases[name], len(pts)
    a, b, n_singular = ops.vertex_components(_t(tets), _t(nbr), _t(case["labels"]), nv)
    want_a, want_b, want_n = m.vertex_components(tets, nbr, case["labels"], nv)
    assert np.array_equal(a.cpu().numpy(), want_a) and np.array_equal(b.cpu().numpy(), want_b) and n_singular == want_n
    got, st = _repair(tets, nbr, case["labels"], nv, cost=case["cost"])
    want, want_st, _, _ = m.repair(tets, nbr, case["labels"], nv, cost=case["cost"])
    assert np.array_equal(got.cpu().numpy(), want)
    _stats_equal(st, want_st)
    assert sorted(np.nonzero(got.cpu().numpy() != case["labels"])[0].tolist()) == case["flips"]      # what the case was built to show
    assert st["singular_after"] == 0
    topo = _topology(pts, tets, nbr, want)
    assert topo is None if name == "all_outside" else topo["watertight"] == 1


def test_malformed_input_is_refused():
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError

    pts, tets, nbr, labels = _scene("u60_n30")
    nv = len(pts)
    c = int(np.nonzero(nbr[:, 0] >= 0)[0][0])

    def both(t, n, lab, cost=None):
        with pytest.raises(DgnnError):
            ops.vertex_components(_t(t), _t(n), _t(lab), nv)
        with pytest.raises(DgnnError):
            _repair(t, n, lab, nv, cost=cost)

    bad = nbr.copy()                                                    # a neighbour that does not name the cell back
    other = int(bad[c, 0])
    bad[other][bad[other] == c] = -1
    both(tets, bad, labels)
    bad = nbr.copy()                                                    # a neighbour that lacks the shared vertices
    far = next(d for d in range(len(tets)) if not set(tets[d]) & set(tets[c]))
    bad[c, 0] = far
    both(tets, bad, labels)
    bad = nbr.copy()
    bad[c, 1] = len(tets)                                               # a cell id out of range
    both(tets, bad, labels)
    bad = tets.copy()
    bad[c, 2] = nv                                                      # a vertex id out of range
    both(bad, nbr, labels)
    bad = labels.copy()
    bad[c] = 2
    both(tets, nbr, bad)
    cost = np.ones(len(tets), dtype=np.int32)
    cost[c] = -1
    with pytest.raises(DgnnError):
        _repair(tets, nbr, labels, nv, cost=cost)
    got, st = _repair(tets, nbr, labels, nv, cost=np.zeros(len(tets), dtype=np.int32))      # zero costs are fine: the cell id decides
    want, want_st, _, _ = m.repair(tets, nbr, labels, nv, cost=np.zeros(len(tets), dtype=np.int32))
    assert np.array_equal(got.cpu().numpy(), want)
    _stats_equal(st, want_st)
