"""The CPU model of the per-facet graph-cut weights (tests/graph_cut_weights_model.py) against closed forms, brute force and its own
extended-precision evaluation; and the library's two new entry points."""
import os

import numpy as np
import pytest

import graph_cut_weights_model as gwm
import mesh_metrics_model as mmm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_closed_forms():
    q = gwm.facet_terms(gwm.regular_pair_scene(), "beta")
    assert abs(q[0] - 2.0 / 3.0) < 1e-14 and not q[1:].any()
    q = gwm.facet_terms(gwm.corner_scene("z0"), "beta")
    assert abs((1 - q[0]) - 1 / np.sqrt(3.0)) < 1e-14 and not q[1:].any()
    q = gwm.facet_terms(gwm.corner_scene("diag"), "beta")
    assert abs((1 - q[0]) + 1.0 / 3.0) < 1e-14 and not q[1:].any()
    # one finite-finite facet: its area is the mean
    assert gwm.facet_terms(gwm.regular_pair_scene(), "area")[0] == 1.0


def test_degenerate_sides_are_neutral_and_counted():
    s = gwm.degenerate_scene()
    q, st = gwm.facet_terms(s, "beta", return_stats=True)
    assert st == {"rows": 3, "neutral_sides": 4}
    # rows 0 and 1: min(cos of the good side, 0); row 2: both sides neutral -> q = 1
    assert q[2] == 1.0 and 1.0 <= q[0] <= 2.0 and 1.0 <= q[1] <= 2.0 and not q[3:].any()
    qa = gwm.facet_terms(s, "area")
    assert np.allclose(qa[:3], [1.5, 1.5, 0.0], rtol=1e-15, atol=0) and not qa[3:].any()


def test_malformed_scenes_raise():
    s = gwm.regular_pair_scene()
    bad = dict(s, facets=s["facets"].copy())
    bad["facets"][0, 1] = 99
    with pytest.raises(gwm.MalformedScene):
        gwm.facet_terms(bad, "beta")
    bad = dict(s, nfacets=s["nfacets"].copy())
    bad["nfacets"][1] = [0, 1]               # a hull facet of cell 0 said to border cell 1 as well
    with pytest.raises(gwm.MalformedScene):
        gwm.facet_terms(bad, "beta")
    flat = dict(s, vertices=np.zeros_like(s["vertices"]))
    with pytest.raises(ZeroDivisionError):
        gwm.facet_terms(flat, "area")


def test_quantise_rounds_half_to_even():
    assert gwm.quantise(np.array([0.05, 0.15, 0.25, 0.35, 1.0]), 10).tolist() == [0, 2, 2, 4, 10]      # 0.5 -> 0, 2.5 -> 2, 3.5 -> 4
    with pytest.raises(ValueError):
        gwm.quantise(np.array([2.0]), 2.0 ** 29)


@pytest.mark.parametrize("uw", [10, 100])
def test_weighted_dinic_oracle_matches_brute_force(uw):
    rng = np.random.default_rng(uw)
    for trial in range(24):
        n = int(rng.integers(2, 13))
        pred = rng.normal(0, 2, (n, 2)).astype(np.float32)
        if trial % 2 == 0:
            pred[::3, 1] = pred[::3, 0]
            pred[1::4] = 0.0
        edges = rng.integers(0, max(n - 1, 1), (int(rng.integers(0, 3 * n + 1)), 2)).astype(np.int32)   # duplicates, self-loops; node n-1 isolated
        w = rng.integers(0, 8, len(edges))
        want, e_want = gwm.brute_force_weighted(pred, edges, uw, w)
        got, e_got, _ = gwm.solve_weighted(pred, edges, uw, w)
        assert np.array_equal(got, want) and e_got == e_want


def test_constant_weights_are_the_potts_model():
    import graph_cut_model as gcm
    rng = np.random.default_rng(5)
    pred = rng.normal(0, 2, (11, 2)).astype(np.float32)
    edges = rng.integers(0, 11, (25, 2)).astype(np.int32)
    assert gwm.brute_force_weighted(pred, edges, 10, np.full(25, 3))[1] == gcm.brute_force(pred, edges, 10, 3)[1]
    lab, e, f = gwm.solve_weighted(pred, edges, 10, np.full(25, 3))
    lab2, e2, f2 = gcm.solve(pred, edges, 10, 3)
    assert np.array_equal(lab, lab2) and (e, f) == (e2, f2)


@pytest.fixture(scope="module", params=[(60, 0), (400, 1), (2000, 2)], ids=lambda p: "%dpts" % p[0])
def scene(request):
    return mmm.random_scene(*request.param)


@pytest.mark.parametrize("kind", gwm.KINDS)
def test_fp64_weights_equal_their_longdouble_evaluation(scene, kind):
    """the integer weights of the fp64 model are those of the same expressions in extended precision: the model is tied to the mathematics
    (the device is then tied to the model bit for bit, tests/test_gpu_graph_cut_weights.py)"""
    q64 = gwm.facet_terms(scene, kind, np.float64)
    qld = gwm.facet_terms(scene, kind, np.longdouble)
    rows = gwm.graph_rows(scene["nfacets"])
    dq = float(np.abs(q64 - qld).max())
    print("%s: %d finite-finite facets, max |dq| = %.3g" % (kind, int(rows.sum()), dq))
    assert not q64[~rows].any()
    for bw in (10, 100, 1000):
        w64, wld = gwm.quantise(q64, bw), gwm.quantise(qld, bw)
        assert np.array_equal(w64, wld), "%d of %d weights differ at bw %d" % (int((w64 != wld).sum()), int(rows.sum()), bw)


def test_library_exports_the_weighted_cut():
    import ctypes
    from dgnn_amd._lib import LIB_PATH, SIGNATURES
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    raw = ctypes.CDLL(LIB_PATH)
    for name in ("dgnn_facet_cut_terms", "dgnn_facet_cut_terms_scratch_bytes", "dgnn_graph_cut_weighted", "dgnn_graph_cut_weighted_scratch_bytes"):
        assert hasattr(raw, name) and name in SIGNATURES, name
    fn = raw.dgnn_facet_cut_terms_scratch_bytes
    fn.restype, fn.argtypes = SIGNATURES["dgnn_facet_cut_terms_scratch_bytes"]
    assert fn(1000) >= 8 * 1000 + 256 and fn(-1) == 0
    fn = raw.dgnn_graph_cut_weighted_scratch_bytes
    fn.restype, fn.argtypes = SIGNATURES["dgnn_graph_cut_weighted_scratch_bytes"]
    ref = raw.dgnn_graph_cut_scratch_bytes
    ref.restype, ref.argtypes = SIGNATURES["dgnn_graph_cut_scratch_bytes"]
    assert fn(1000, 2000) == ref(1000, 2000) > 0
