"""The CPU model of the Delaunay contract (tests/delaunay_model.py) against scipy's triangulations: it accepts them in general position and
rejects them after a flip, after a removed cell, and on a grid (flat cells).  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from delaunay_model import (canonical, certificate, cube_face_points, grid_points, flip23, insphere_signs, orient_signs, strictly_delaunay,
                            tables,
                            uniform_points)

scipy_spatial = pytest.importorskip("scipy.spatial")


def test_the_insphere_sign_is_the_distance_to_the_circumcentre():
    rng = np.random.default_rng(0)
    pts = rng.integers(-20, 21, size=(200, 5, 3)).astype(np.float64)
    got = insphere_signs(*(pts[:, i] for i in range(5)))
    for q, s in zip(pts, got):
        a, b, c, d, e = ([Fraction(int(x)) for x in r] for r in q)
        # the centre x solves 2 (p - a) . x = |p|^2 - |a|^2 for p = b, c, d (Cramer)
        rows = [[2 * (p[i] - a[i]) for i in range(3)] for p in (b, c, d)]
        rhs = [sum(x * x for x in p) - sum(x * x for x in a) for p in (b, c, d)]
        det = lambda m: (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                         + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
        D = det(rows)
        if D == 0:
            assert s == 0
            continue
        x = [det([[rhs[r] if j == i else rows[r][j] for j in range(3)] for r in range(3)]) / D for i in range(3)]
        r2 = sum((a[i] - x[i]) ** 2 for i in range(3))
        d2 = sum((e[i] - x[i]) ** 2 for i in range(3))
        assert s == (d2 < r2) - (d2 > r2)


def test_the_filtered_and_the_exact_stage_agree_on_float_input():
    rng = np.random.default_rng(1)
    pts = rng.random((300, 5, 3))
    fast = insphere_signs(*(pts[:, i] for i in range(5)))
    # the same cases scaled by 2^-140: the filter's absolute term sends every one to the Fractions, the signs are those of the unscaled cases
    slow = insphere_signs(*(pts[:, i] * 2.0 ** -140 for i in range(5)))
    assert np.array_equal(fast, slow) and np.all(fast != 0)
    assert np.array_equal(orient_signs(pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]),
                          orient_signs(*(pts[:, i] * 2.0 ** -250 for i in range(4))))


@pytest.fixture(scope="module", params=["uniform", "cube_faces"])
def scipy_case(request):
    P = uniform_points(300) if request.param == "uniform" else cube_face_points(300)
    return P, scipy_spatial.Delaunay(P).simplices


def test_the_model_accepts_scipy_in_general_position(scipy_case):
    P, simp = scipy_case
    inside, on, flat = strictly_delaunay(P, simp)
    assert (inside, on, flat) == (0, 0, 0)
    t, nb, hf = tables(P, simp[orient_signs(P[simp[:, 0]], P[simp[:, 1]], P[simp[:, 2]], P[simp[:, 3]]) != 0])
    assert certificate(P, t, nb, hf) == []


def test_the_model_rejects_a_flip_and_a_missing_cell(scipy_case):
    P, simp = scipy_case
    t, nb, hf = tables(P, simp)
    flipped = tables(P, flip23(t, nb))
    assert certificate(P, *flipped) != []
    missing = tables(P, np.delete(t, len(t) // 2, axis=0))
    assert certificate(P, *missing) != []


def test_the_model_rejects_scipys_grid_cells():
    P = grid_points(4)
    simp = scipy_spatial.Delaunay(P).simplices
    flat = int((orient_signs(P[simp[:, 0]], P[simp[:, 1]], P[simp[:, 2]], P[simp[:, 3]]) == 0).sum())
    assert flat > 0
    assert any("strictly positive" in s for s in certificate(P, *tables(P, simp)))


def test_canonical_keeps_the_orientation():
    P = uniform_points(40)
    simp = scipy_spatial.Delaunay(P).simplices
    t = canonical(tables(P, simp)[0])
    assert np.all(orient_signs(P[t[:, 0]], P[t[:, 1]], P[t[:, 2]], P[t[:, 3]]) > 0)
    assert np.all(t[:, 0] == t.min(axis=1)) and np.array_equal(t, np.array(sorted(map(tuple, t))))
