"""The point-to-mesh distance rule (include/dgnn_hip.h) as tests/mesh_distance_model.py states it: its accuracy against the same
rule in exact rationals, its ties, its degenerate faces, the restated device search against all pairs, and the fold model.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import mesh_contains_model as mc
import mesh_distance_model as md

# the worst |sqrt(d2) - d_exact| measured over 10 000 cases of accuracy_cases (seed 0) was 31.1 units of 2^-52 x (largest coordinate
# magnitude of the case), at a point in the plane of a thin random triangle (the sine of its angle at v0 is 0.0055; the normal's direction is
# known to about 3 u / sine); the 9 999 others stay below 3.2.  The bound is four times the worst, for other seeds.
ACCURACY_BOUND_UNITS = 4 * 31.1


def accuracy_cases(n, seed):
    """(point, triangle) cases in the families of DESIGN §30: random triangles; points on planes, edges and vertices and 1e-9 off them; integer
    lattices with degenerate faces; needles"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        fam = k % 10
        if fam < 4:
            yield rng.uniform(-2, 2, 3), rng.uniform(-1, 1, (3, 3))
        elif fam < 7:
            tri = rng.uniform(-1, 1, (3, 3))
            w = rng.dirichlet((1, 1, 1))
            m = (k // 10) % 5
            if m == 0:
                w = np.array([w[0], 1 - w[0], 0.0])
            elif m == 1:
                w = np.array([1.0, 0.0, 0.0])
            elif m == 2:
                w = np.array([1.2, -0.1, -0.1])
            p = w @ tri
            if m == 4:
                p = p + 1e-9 * rng.normal(size=3)
            yield p, tri
        elif fam < 9:
            yield rng.integers(-4, 5, 3).astype(float), rng.integers(-3, 4, (3, 3)).astype(float)
        else:
            a, b = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
            yield rng.uniform(-1, 1, 3), np.array([a, b, a + (b - a) * rng.uniform() + 1e-12 * rng.normal(size=3)])


def accuracy_units(p, tri):
    got = md.face_rule(tuple(float(x) for x in p), [tuple(float(x) for x in t) for t in tri])[0]
    exact = md.face_rule(tuple(Fraction(float(x)) for x in p), [tuple(Fraction(float(x)) for x in t) for t in tri])[0]
    scale = max(np.abs(p).max(), np.abs(tri).max())
    return abs(np.sqrt(got) - md.sqrt_fraction(exact)) / (2.0 ** -52 * scale)


def test_model_against_the_rule_in_rationals():
    worst = max(accuracy_units(p, tri) for p, tri in accuracy_cases(2000, seed=1))
    print("worst |sqrt(d2) - d_exact| = %.2f units of 2^-52 x the largest coordinate magnitude" % worst)
    assert worst <= ACCURACY_BOUND_UNITS


def test_scalar_and_all_pairs_forms_agree():
    for v, f in (mc.cube(0.2, 0.8), md.degenerate_mesh(), mc.tetrahedron()):
        q = md.query_points(v, f, 60, seed=2)
        d2, face, closest, region = md.distance(v, f, q)
        for i in range(len(q)):
            want = md.distance_scalar(v, f, q[i])
            assert (d2[i], face[i], tuple(closest[i]), region[i]) == (want[0], want[1], tuple(want[2]), want[3])


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second, region", [((1, 0, 3), 1), ((0, 1, 3), 1), ((3, 1, 0), 2)])
def test_faces_sharing_an_edge_tie_for_both_windings(second, region):
    rng = np.random.default_rng(3)
    n_tied = 0
    for _ in range(200):
        v = rng.uniform(-1, 1, (4, 3))
        faces = np.array([[0, 1, 2], second], dtype=np.int32)
        w = rng.uniform(0.05, 0.95)
        mid = (1 - w) * v[0] + w * v[1]
        # a point whose closest point is on the shared edge (0, 1): off the edge, away from both faces
        away = -((v[2] - mid) / np.linalg.norm(v[2] - mid) + (v[3] - mid) / np.linalg.norm(v[3] - mid))
        e = v[1] - v[0]
        away -= (away @ e) / (e @ e) * e
        p = mid + 0.3 * away
        tri = [[tuple(float(x) for x in v[i]) for i in fc] for fc in faces]
        a, b = md.face_rule(tuple(p), tri[0], tuple(faces[0])), md.face_rule(tuple(p), tri[1], tuple(int(i) for i in faces[1]))
        if a[2] == 1 and b[2] == region:          # both closest on the shared edge (the construction can fail for a sharp pair)
            n_tied += 1
            assert a[0] == b[0] and a[1] == b[1]          # the same bits, whichever way the second face runs along the edge
            assert md.distance(v, faces, p[None])[1][0] == 0
            assert md.distance(v, faces[::-1], p[None])[1][0] == 0          # the lower INDEX wins, whichever face it is
    assert n_tied >= 50


def test_faces_sharing_a_vertex_tie_and_the_lower_face_wins():
    v = np.array([[0.1, 0.2, 0.3], [1.0, 0.1, 0.0], [0.2, 1.1, 0.1], [-1.0, 0.3, -0.2], [-0.1, -1.2, 0.1]])
    faces = np.array([[3, 4, 0], [0, 1, 2]], dtype=np.int32)
    p = v[0] + np.array([-0.01, -0.02, 0.5])
    d2, face, closest, region = md.distance(v, faces, np.array([p, v[0]]))
    assert list(face) == [0, 0] and list(region) == [6, 6] and np.array_equal(closest, [v[0], v[0]]) and d2[1] == 0.0
    d2r, facer, _, regionr = md.distance(v, faces[::-1], np.array([p, v[0]]))
    assert np.array_equal(d2, d2r) and list(facer) == [0, 0] and list(regionr) == [4, 4]


def test_duplicate_face_and_cube_centre():
    v, f = mc.cube(0.0, 4.0)
    q = md.query_points(v, f, 100, seed=4)
    d2, face, closest, region = md.distance(v, np.concatenate([f, f]), q)
    want = md.distance(v, f, q)
    assert np.array_equal(face, want[1]) and np.array_equal(d2, want[0]) and face.max() < len(f)
    d2, face, closest, region = md.distance(v, f, np.array([[2.0, 2.0, 2.0]]))
    assert d2[0] == 4.0 and face[0] == 0          # six squares at the same distance: the lowest face


# ---- degenerate faces ------------------------------------------------------------------------------------------------------------------
def test_degenerate_faces_are_their_segments_or_point():
    rng = np.random.default_rng(5)
    v = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.5, -1.0, 0.25]])
    q = rng.uniform(-3, 7, (200, 3))
    for face, ends in (([0, 1, 2], (0, 2)), ([0, 2, 1], (0, 2)), ([3, 1, 3], (1, 3)), ([1, 1, 3], (1, 3)), ([3, 3, 3], (3, 3))):
        d2, _, closest, region = md.distance(v, np.array([face], dtype=np.int32), q)
        assert np.isfinite(d2).all() and np.isfinite(closest).all() and (region > 0).all()
        for i in range(0, len(q), 5):
            u, w = (tuple(float(x) for x in v[k]) for k in ends)
            exact = md.segment_rule(tuple(Fraction(float(x)) for x in q[i]), tuple(Fraction(x) for x in u), tuple(Fraction(x) for x in w))[0]
            assert abs(np.sqrt(d2[i]) - md.sqrt_fraction(exact)) <= 16 * 2.0 ** -52 * 7.0
    d2, _, closest, region = md.distance(v, np.array([[3, 3, 3]], dtype=np.int32), q)
    assert np.array_equal(closest, np.tile(v[3], (len(q), 1))) and (region == 4).all()


# ---- the device's search, restated ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["cube", "degenerate", "flat", "unequal"])
def test_restated_search_equals_all_pairs(mesh):
    v, f = {"cube": lambda: mc.cube(0.2, 0.8), "degenerate": md.degenerate_mesh, "flat": md.flat_mesh, "unequal": lambda: md.unequal_mesh(40)}[mesh]()
    q = md.query_points(v, f, 80, seed=6)
    want = md.distance(v, f, q)
    for R in (1, 2, 7):
        got = md.distance_grid(v, f, q, R)
        for a, b in zip(got[:4], want):
            assert np.array_equal(a, b)


def test_restated_search_reads_deep_shells_on_a_large_mesh():
    """28 560 faces, queries 100 extents outside the box: tens of shells, stopped by the bound with its box terms, equal to all pairs"""
    v, f = md.uv_sphere(120, 120)
    q = md.deep_queries()["outside"][:12]
    got = md.distance_grid(v, f, q, 60)
    for a, b in zip(got[:4], md.distance(v, f, q, chunk=16)):
        assert np.array_equal(a, b)
    assert 30 <= got[4][0] < 60 and got[4][1] >= 12 * 8


# ---- the fold ------------------------------------------------------------------------------------------------------------------------
def test_fold_model():
    rng = np.random.default_rng(7)
    d = rng.random(600)
    s, sc, m, k = md.fold(d, -d, thresholds=(d[3], 0.5, 2.0, -1.0))
    parts = [sum(float(x) for x in d[a:a + 256]) for a in (0, 256, 512)]          # chunks of 256, then the chunk totals serially
    want = (parts[0] + parts[1]) + parts[2]
    assert s == want and sc == want and m == d.max()
    assert k == [int((d <= d[3]).sum()), int((d <= 0.5).sum()), 600, 0] and k[0] >= 1          # a threshold equal to a distance counts it
    assert md.fold(np.zeros(0), None, (1.0,)) == (0.0, 0.0, 0.0, [0])
    out = md.metrics_from_folds((1.0, 3.0, 0.5, [2]), 4, (2.0, 1.0, 0.75, [0]), 4, (0.1,))
    assert out == {"accuracy": 0.25, "completeness": 0.5, "chamfer_mesh": 0.375, "hausdorff": 0.75, "precision@0.1": 0.5, "recall@0.1": 0.0,
                   "fscore@0.1": 0.0, "normal_consistency": 0.5}
