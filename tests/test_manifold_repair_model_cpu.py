"""The manifold repair's rule on the CPU (tests/manifold_repair_model.py), on scipy triangulations: the criterion against the
face-level check of the extracted interface, the termination argument and what the mark is for, and hand-built labellings whose outcome
can be reasoned out.  The device is held to this model in tests/test_gpu_manifold_repair.py."""
import numpy as np
import pytest

import manifold_repair_model as m
from helpers import gold

_CACHE = {}


def _scene(name, form):
    """form "scipy": the cells as scipy numbers them; "canonical": in the order and row form of ops.delaunay (for points in general position
    the very cells the device tests run on)"""
    if (name, form) not in _CACHE:
        points, labels, clean = m.SCENES[name]
        pts = points()
        tets, nbr = m.scipy_scene(pts)
        if form == "canonical":
            tets, nbr = m.canonical_order(pts, tets, nbr)
        _CACHE[name, form] = (tets, nbr, labels(pts, tets), len(pts), clean)
    return _CACHE[name, form]


def _no_singular_iff_manifold(tets, nbr, labels, nv):
    a, b, n_singular = m.vertex_components(tets, nbr, labels, nv)
    fc = m.face_check(tets, nbr, labels)
    assert fc["boundary_edges"] == 0
    assert (n_singular == 0) == (fc["nonmanifold_edges"] == 0 and fc["multi_fan_vertices"] == 0), (n_singular, fc)
    return n_singular


@pytest.mark.parametrize("name", list(m.SCENES))
@pytest.mark.parametrize("cost_mode", ["count", "margin"])
@pytest.mark.parametrize("form", ["scipy", "canonical"])
def test_criterion_equals_the_face_check_and_the_rule_terminates(name, cost_mode, form):
    tets, nbr, labels, nv, clean = _scene(name, form)
    cost = None if cost_mode == "count" else m.margin_cost(len(tets))
    before = _no_singular_iff_manifold(tets, nbr, labels, nv)
    out, st, flipped, history = m.repair(tets, nbr, labels, nv, cost=cost)
    after = _no_singular_iff_manifold(tets, nbr, out, nv)
    assert st["singular_before"] == before and st["singular_after"] == after
    assert st["max_flips_of_a_cell"] <= 1 and st["rounds"] <= st["flipped_cells"] and st["rounds"] == len(history)
    assert st["flipped_cells"] == int(flipped.sum()) == int((out != labels).sum())
    assert st["moves"] >= st["rounds"]                                   # the lowest vertex with a move wins in every round
    if clean:
        assert after == 0
    if name == "u300_n50":
        assert after > 0                                                 # stuck vertices are reported, not hidden
    for r in (1, 2, 3):                                                  # max_rounds only stops early
        if r <= len(history):
            part, st_r, _, _ = m.repair(tets, nbr, labels, nv, cost=cost, max_rounds=r)
            assert np.array_equal(part, history[r - 1]) and st_r["rounds"] == r


def test_without_the_mark_the_rule_oscillates():
    g = gold("manifold_oscillation.npz")
    tets, nbr, labels, cost = (g[k].astype(np.int32) for k in ("tetrahedra", "neighbors", "labels", "cost"))
    nv = int(g["n_vertices"])
    _, free, _, _ = m.repair(tets, nbr, labels, nv, cost=cost, mark=False, max_rounds=200)
    assert free["rounds"] == 200 and free["max_flips_of_a_cell"] > 100      # still flipping, the same cells again and again
    out, st, _, _ = m.repair(tets, nbr, labels, nv, cost=cost)
    assert st["singular_after"] == 0 and st["rounds"] < 40 and st["max_flips_of_a_cell"] == 1
    assert _no_singular_iff_manifold(tets, nbr, out, nv) == 0


@pytest.fixture(scope="module")
def hand():
    pts = m.uniform_points(60, 7)
    tets, nbr = m.scipy_scene(pts)
    return tets, nbr, len(pts), m.hand_cases(tets, nbr)


@pytest.mark.parametrize("name", ["edge_pair", "edge_pair_cost", "vertex_pair", "hull_inside", "all_inside", "all_outside", "pocket", "larger_cheaper",
                                  "larger_dearer"])
def test_hand_built_cases(hand, name):
    tets, nbr, nv, cases = hand
    case = cases[name]
    a, b, n_singular = m.vertex_components(tets, nbr, case["labels"], nv)
    assert (n_singular > 0) == bool(case["flips"])
    out, st, flipped, _ = m.repair(tets, nbr, case["labels"], nv, cost=case["cost"])
    assert sorted(np.nonzero(out != case["labels"])[0].tolist()) == case["flips"]
    assert st["singular_after"] == 0 and st["rounds"] == (1 if case["flips"] else 0) and st["moves"] == st["rounds"]
    assert _no_singular_iff_manifold(tets, nbr, out, nv) == 0
    if name == "all_inside":
        hull = sorted(m.hull_vertices(tets, nbr))
        assert (a == 1).all() and (b[hull] == 1).all() and b.sum() == len(hull)      # the outside of a hull vertex is the infinite cell alone
    if name == "all_outside":
        assert (a == 0).all() and (b == 1).all()
    if name == "pocket":
        assert a.max() == 1 and b.max() == 1 and b.sum() > 0
