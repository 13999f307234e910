"""Per-facet graph-cut weights on the device (ops.facet_cut_terms / dgnn_facet_cut_terms) and the cut that takes them
(ops.weighted_graph_cut / dgnn_graph_cut_weighted, generate's ``graph_cut.binary_term``) against the CPU model
(tests/graph_cut_weights_model.py): q bit for bit, weights, labels, energy and flow equal."""
import os

import numpy as np
import pytest
import torch

import graph_cut_model as gcm
import graph_cut_weights_model as gwm
import mesh_metrics_model as mmm
from dgnn_amd.config import Config
from helpers import gold

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- scenes and their model terms, computed once ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    out = {"regular": gwm.regular_pair_scene(), "corner_z0": gwm.corner_scene("z0"), "corner_diag": gwm.corner_scene("diag"),
           "400": mmm.random_scene(400, 1), "2000": mmm.random_scene(2000, 2)}
    for s in out.values():
        s["rows"] = gwm.graph_rows(s["nfacets"])
        s["edges"] = np.ascontiguousarray(s["nfacets"][s["rows"]], dtype=np.int32)
        both = {k: gwm.facet_terms(s, k, return_stats=True) for k in gwm.KINDS}
        s["q"], s["stats"] = {k: both[k][0] for k in gwm.KINDS}, {k: both[k][1] for k in gwm.KINDS}
    return out


def _terms(scene, kind, bw, **kw):
    from dgnn_amd import ops
    return ops.facet_cut_terms(scene["vertices"], scene["tetrahedra"], scene["facets"], scene["nfacets"], kind, bw, **kw)


def _cut(pred, edges, uw, weights, **kw):
    from dgnn_amd import ops
    out = ops.weighted_graph_cut(torch.from_numpy(pred).to(DEV), torch.from_numpy(np.asarray(edges, dtype=np.int32).reshape(-1, 2)).to(DEV), uw,
                                 torch.as_tensor(weights), **kw)
    assert out[0].is_cuda and out[0].dtype == torch.int32
    return (out[0].cpu().numpy(),) + tuple(out[1:])


# ---- the terms -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("regular", "beta"), ("corner_z0", "beta"), ("corner_diag", "beta"), ("regular", "area"), ("400", "area"),
                                       ("400", "beta")])
def test_terms_match_the_model_bit_for_bit(scenes, name, kind):
    s = scenes[name]
    for bw in (10, 100.5):
        w, q, st = _terms(s, kind, bw, return_q=True)
        assert w.is_cuda and w.dtype == torch.int32 and q.dtype == torch.float64
        q, w = q.cpu().numpy(), w.cpu().numpy()
        want_w = gwm.quantise(s["q"][kind], bw)
        assert np.array_equal(q.view(np.int64), s["q"][kind].view(np.int64)), "max |dq| = %g" % np.abs(q - s["q"][kind]).max()
        assert np.array_equal(w, want_w)
        assert not q[~s["rows"]].any() and not w[~s["rows"]].any() and (~s["rows"]).any()          # hull facets give 0
        assert st == {"rows": int(s["rows"].sum()), "neutral_sides": s["stats"][kind]["neutral_sides"], "zero_weights": int((want_w[s["rows"]] == 0).sum()),
                      "max_weight": int(want_w.max())}
    w2, _ = _terms(s, kind, 10)            # without q
    assert np.array_equal(w2.cpu().numpy(), gwm.quantise(s["q"][kind], 10))


def test_closed_forms_on_the_device(scenes):
    q = _terms(scenes["regular"], "beta", 1, return_q=True)[1].cpu().numpy()
    assert abs(q[0] - 2.0 / 3.0) < 1e-14
    q = _terms(scenes["corner_z0"], "beta", 1, return_q=True)[1].cpu().numpy()
    assert abs((1 - q[0]) - 1 / np.sqrt(3.0)) < 1e-14
    q = _terms(scenes["corner_diag"], "beta", 1, return_q=True)[1].cpu().numpy()
    assert abs((1 - q[0]) + 1.0 / 3.0) < 1e-14


def test_degenerate_cells_and_facets_are_neutral():
    s = gwm.degenerate_scene()
    want_q, want_st = gwm.facet_terms(s, "beta", return_stats=True)
    w, q, st = _terms(s, "beta", 10, return_q=True)
    assert np.array_equal(q.cpu().numpy().view(np.int64), want_q.view(np.int64)) and np.array_equal(w.cpu().numpy(), gwm.quantise(want_q, 10))
    assert st["rows"] == want_st["rows"] == 3 and st["neutral_sides"] == want_st["neutral_sides"] == 4
    assert float(q[2]) == 1.0 and int(w[2]) == 10                   # both sides of the zero-area facet are right angles
    w, q, st = _terms(s, "area", 10, return_q=True)
    want_q = gwm.facet_terms(s, "area")
    assert np.array_equal(q.cpu().numpy().view(np.int64), want_q.view(np.int64)) and w.cpu().tolist() == [15, 15, 0, 0, 0]
    assert st == {"rows": 3, "neutral_sides": 0, "zero_weights": 1, "max_weight": 15}


def test_bad_scenes_raise():
    from dgnn_amd._lib import DgnnError
    s = gwm.regular_pair_scene()
    bad = dict(s, facets=s["facets"].copy())
    bad["facets"][0, 1] = 99                                          # a facet's vertex id out of range
    for kind in gwm.KINDS:
        with pytest.raises(DgnnError, match="out of range"):
            _terms(bad, kind, 10)
    bad = dict(s, tetrahedra=s["tetrahedra"].copy())
    bad["tetrahedra"][1, 3] = -7                                      # a cell's vertex id out of range
    with pytest.raises(DgnnError, match="out of range"):
        _terms(bad, "beta", 10)
    bad = dict(s, nfacets=s["nfacets"].copy())
    bad["nfacets"][0, 1] = 5                                          # a cell id out of range
    with pytest.raises(DgnnError, match="out of range"):
        _terms(bad, "beta", 10)
    bad = dict(s, nfacets=s["nfacets"].copy())
    bad["nfacets"][1] = [0, 1]                                        # a hull facet of cell 0 said to border cell 1 as well
    with pytest.raises(DgnnError, match="not a face"):
        _terms(bad, "beta", 10)
    flat = dict(s, vertices=np.zeros_like(s["vertices"]))
    with pytest.raises(DgnnError, match="mean facet area"):
        _terms(flat, "area", 10)
    with pytest.raises(DgnnError, match="2\\^30"):
        _terms(s, "beta", 2.0 ** 31)
    for bw in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _terms(s, "beta", bw)
    with pytest.raises(ValueError):
        _terms(s, "gamma", 10)
    # a good call after the failed ones still works
    assert int(_terms(s, "area", 10)[0][0]) == 10


# ---- the weighted cut ------------------------------------------------------------------------------------------------------------------
def _check_brute(pred, edges, uw, weights):
    edges = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    got, e_got, f_got = _cut(pred, edges, uw, weights)
    want, e_want = gwm.brute_force_weighted(pred, edges, uw, weights)
    D = gcm.unary_costs(pred, uw)
    assert e_got == f_got + int(np.minimum(D[:, 0], D[:, 1]).sum())
    assert np.array_equal(got, want) and e_got == e_want


@pytest.mark.parametrize("uw,wmax", [(10, 8), (10, 200), (100, 8), (100, 200)])
def test_tiny_graphs_match_brute_force(uw, wmax):
    rng = np.random.default_rng(uw * 1000 + wmax)
    for trial in range(16):                                            # 4 x 16 = 64 graphs
        n = int(rng.integers(2, 13))
        pred = rng.normal(0, 2, (n, 2)).astype(np.float32)
        if trial % 2 == 0:
            pred[::3, 1] = pred[::3, 0]          # exact ties in the unary cost
            pred[1::4] = 0.0                     # costs of zero
        if trial % 5 == 0:
            pred = -np.abs(pred) - 0.5           # all costs negative
        edges = rng.integers(0, n, (int(rng.integers(0, 3 * n + 1)), 2)).astype(np.int32)   # duplicates, self-loops, isolated cells
        weights = rng.integers(0, wmax, len(edges))
        weights[rng.random(len(edges)) < 0.2] = 0
        _check_brute(pred, edges, uw, weights)


def test_tiny_graph_structure_cases():
    pred = np.array([[0.3, 0.1], [0.1, 0.3], [0.2, 0.2], [-1.0, 0.5], [0.0, 0.0], [2.0, -2.0], [0.05, 0.15]], dtype=np.float32)
    rng = np.random.default_rng(0)
    for edges in ([], [[0, 1], [0, 1], [1, 1]], [[2, 3], [3, 2], [4, 4], [0, 6]], [[i, j] for i in range(7) for j in range(7)]):
        for scale in (0, 1, 10, 100):
            weights = rng.integers(0, 4, len(edges)) * scale            # scale 0: the all-zero vector
            _check_brute(pred, edges, 10, weights)
    # no capacity anywhere: the arg-min of the unary costs, ties to inside
    edges = [[i, j] for i in range(7) for j in range(7)]
    got, e_got, f_got = _cut(pred, edges, 10, np.zeros(len(edges), dtype=np.int64))
    D = gcm.unary_costs(pred, 10)
    assert np.array_equal(got, (D[:, 1] < D[:, 0]).astype(np.int32)) and e_got == int(np.minimum(D[:, 0], D[:, 1]).sum())


@pytest.mark.parametrize("name,kind,field", [("400", "area", "coherent"), ("400", "area", "noise"), ("400", "beta", "coherent"), ("400", "beta", "noise"),
                                             ("2000", "beta", "coherent")])
def test_delaunay_facet_graph_matches_dinic(scenes, name, kind, field):
    s = scenes[name]
    n = len(s["tetrahedra"])
    pred = gcm.coherent_logits(mmm.centroids(s), seed=1) if field == "coherent" else gcm.noise_logits(n, seed=1)
    w_all, st = _terms(s, kind, 10)
    weights = w_all[torch.from_numpy(s["rows"]).to(DEV)]
    assert np.array_equal(weights.cpu().numpy(), gwm.quantise(s["q"][kind], 10)[s["rows"]]) and len(np.unique(weights.cpu().numpy())) > 2
    got, e_got, f_got = _cut(pred, s["edges"], 10, weights)
    want, e_want, f_want = gwm.solve_weighted(pred, s["edges"], 10, weights.cpu().numpy())
    assert np.array_equal(got, want) and e_got == e_want and f_got == f_want
    assert e_got == gwm.energy_weighted(got, gcm.unary_costs(pred, 10), s["edges"], weights.cpu().numpy())
    assert 0 < got.sum() < n


def test_constant_weights_are_binary_graph_cut(scenes):
    from dgnn_amd import ops
    s = scenes["2000"]
    pred = gcm.noise_logits(len(s["tetrahedra"]), seed=3)
    p_dev, e_dev = torch.from_numpy(pred).to(DEV), torch.from_numpy(s["edges"]).to(DEV)
    for w in (1, 7):
        a = ops.binary_graph_cut(p_dev, e_dev, 10, w, return_stats=True)
        b = ops.weighted_graph_cut(p_dev, e_dev, 10, torch.full((len(s["edges"]),), w, dtype=torch.int32), return_stats=True)
        assert torch.equal(a[0], b[0]) and a[1:] == b[1:] and a[3]["steps"] > 0


def test_reruns_are_bit_identical(scenes):
    s = scenes["2000"]
    pred = gcm.noise_logits(len(s["tetrahedra"]), seed=4)
    runs = []
    for _ in range(2):
        w, q, st = _terms(s, "beta", 10, return_q=True)
        cut = _cut(pred, s["edges"], 10, w[torch.from_numpy(s["rows"]).to(DEV)], return_stats=True)
        runs.append((w.cpu().numpy(), q.cpu().numpy().view(np.int64), st, cut))
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.array_equal(a[3][0], b[3][0]) and a[3][1:] == b[3][1:]
    wa = _terms(s, "area", 10, return_q=True)
    wb = _terms(s, "area", 10, return_q=True)
    assert torch.equal(wa[0], wb[0]) and torch.equal(wa[1].view(torch.int64), wb[1].view(torch.int64)) and wa[2] == wb[2]


def test_argument_errors_raise():
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    pred = np.random.default_rng(0).normal(0, 1, (6, 2)).astype(np.float32)
    pred[1] = [1.0, 0.0]                                                                              # a terminal capacity of 10 at node 1
    p_dev = torch.from_numpy(pred).to(DEV)
    edges = np.array([[0, 1], [2, 3], [1, 2]], dtype=np.int32)
    with pytest.raises(DgnnError, match="weight < 0"):
        ops.weighted_graph_cut(p_dev, edges, 10, [1, -1, 1])
    with pytest.raises(DgnnError, match="weight < 0"):
        ops.weighted_graph_cut(p_dev, np.array([[0, 1], [2, 2]], dtype=np.int32), 10, [1, -1])        # on a self-loop too
    with pytest.raises(ValueError):
        ops.weighted_graph_cut(p_dev, edges, 10, [1, 1])                                              # wrong length
    with pytest.raises(ValueError):
        ops.weighted_graph_cut(p_dev, edges, 10, [[1, 1, 1]])
    with pytest.raises(ValueError):
        ops.weighted_graph_cut(p_dev, edges, 10, [1.0, 1.0, 1.0])
    with pytest.raises(DgnnError, match="overflow"):
        ops.weighted_graph_cut(p_dev, edges, 10, [2 ** 30 - 1, 1, 2 ** 30 - 1])                       # node 1: 10 + 2 (2^30 - 1) > INT32_MAX
    with pytest.raises(DgnnError, match="overflow"):
        ops.weighted_graph_cut(p_dev, edges, 10, [0, 2 ** 30, 0])                                     # an arc's residual can reach 2 w
    with pytest.raises(DgnnError):
        ops.weighted_graph_cut(p_dev, np.array([[0, 6]], dtype=np.int32), 10, [1])
    from dgnn_amd.processing.generate_mesh import graph_cut_gpu
    clf = Config(graph_cut=Config(unary_weight=10, binary_weight=1))
    with pytest.raises(ValueError):
        graph_cut_gpu(np.zeros(6, dtype=np.int32), pred, edges, clf, row_weights=[1, 1])
    # a good call after the failed ones still works; 2^30 - 1 on one arc of a node with small terminals fits
    got = graph_cut_gpu(np.zeros(6, dtype=np.int32), pred, edges, clf, row_weights=[3, 0, 2])
    assert isinstance(got, np.ndarray) and np.array_equal(got, gwm.brute_force_weighted(pred, edges, 10, [3, 0, 2])[0])
    got, _, _ = _cut(pred, edges, 10, [2 ** 29, 1, 0])
    assert np.array_equal(got, gwm.brute_force_weighted(pred, edges, 10, [2 ** 29, 1, 0])[0])


# ---- generate ----------------------------------------------------------------------------------------------------------------------------
def _scene(tmp_path):
    g = gold("genmesh_f4_small.npz")
    os.makedirs(os.path.join(str(tmp_path), "gt"), exist_ok=True)
    np.savez(os.path.join(str(tmp_path), "gt", "0_3dt.npz"), vertices=g["vertices"], tetrahedra=g["tetrahedra"], facets=g["facets"], nfacets=g["nfacets"])
    data = Config(path=str(tmp_path), gtfile="gt/0", filename="0", id="", category="", infinite=torch.from_numpy(g["infinite"]))
    return g, data


def _clf(bw, term="absent", solver="gpu", graph_cut=1):
    gc = Config(unary_weight=10.0, binary_weight=bw, binary_type="beta")
    if solver is not None:
        gc.solver = solver
    if term != "absent":
        gc.binary_term = term
    return Config(temp=Config(graph_cut=graph_cut, fix_orientation=0, metrics=[], device=DEV), graph_cut=gc)


@pytest.mark.parametrize("term", ["beta", "area"])
def test_generate_with_facet_terms(tmp_path, capsys, term):
    from dgnn_amd.processing.generate_mesh import generate
    g, data = _scene(tmp_path)
    fin, nf = g["infinite"] == 0, g["nfacets"]
    rows = (nf >= 0).all(1)
    weights = gwm.quantise(gwm.facet_terms(g, term), 10.0)[rows]
    want_labels, _, _ = gwm.solve_weighted(g["prediction"][fin], nf[rows], 10.0, weights)
    want_faces = gcm.interface_faces(want_labels, nf, g["facets"])
    for pred in (torch.from_numpy(g["prediction"]).to(DEV), torch.from_numpy(g["prediction"])):
        mesh, ev = generate(data, pred, _clf(10.0, term))
        assert ev == {} and np.array_equal(np.asarray(mesh.faces), want_faces)
    assert "WARNING" not in capsys.readouterr().out
    # the test sees the weights: neither the raw arg-max nor the uniform cut gives these faces
    uniform = gcm.interface_faces(gcm.solve(g["prediction"][fin], nf[rows], 10.0, 10.0)[0], nf, g["facets"])
    assert not np.array_equal(want_faces, g["faces"]) and not np.array_equal(want_faces, uniform)


def test_generate_uniform_is_todays_path(tmp_path, capsys):
    from dgnn_amd.processing.generate_mesh import generate
    g, data = _scene(tmp_path)
    fin, nf = g["infinite"] == 0, g["nfacets"]
    want = gcm.interface_faces(gcm.solve(g["prediction"][fin], nf[(nf >= 0).all(1)], 10.0, 10.0)[0], nf, g["facets"])
    pred = torch.from_numpy(g["prediction"]).to(DEV)
    for term in ("absent", None, "uniform"):
        mesh, _ = generate(data, pred, _clf(10.0, term))
        assert np.array_equal(np.asarray(mesh.faces), want)
    assert "WARNING" not in capsys.readouterr().out


def test_generate_rejects_bad_binary_terms(tmp_path, capsys):
    from dgnn_amd.processing.generate_mesh import generate
    g, data = _scene(tmp_path)
    pred = torch.from_numpy(g["prediction"]).to(DEV)
    with pytest.raises(ValueError, match="binary_term"):
        generate(data, pred, _clf(10.0, "gamma"))
    with pytest.raises(ValueError, match="solver"):
        generate(data, pred, _clf(10.0, "beta", solver=None))
    with pytest.raises(ValueError, match="solver"):
        generate(data, pred, _clf(10.0, "area", solver="cpu"))
    assert "WARNING" not in capsys.readouterr().out
    # the graph cut switched off: the key is not looked at
    mesh, _ = generate(data, pred, _clf(10.0, "gamma", graph_cut=0))
    assert np.array_equal(np.asarray(mesh.faces), g["faces"])


def test_generate_falls_back_when_a_device_step_fails(tmp_path, capsys):
    from dgnn_amd.processing.generate_mesh import generate
    g, data = _scene(tmp_path)
    pred = torch.from_numpy(g["prediction"]).to(DEV)
    mesh, _ = generate(data, pred, _clf(-1.0, "beta"))                     # the terms refuse a negative binary_weight
    assert np.array_equal(np.asarray(mesh.faces), g["faces"])
    assert "WARNING: Graph cut for 0 didn't work" in capsys.readouterr().out
    mesh, _ = generate(data, pred, _clf(2.0 ** 31, "area"))                # weights beyond 2^30
    assert np.array_equal(np.asarray(mesh.faces), g["faces"])
    assert "WARNING: Graph cut for 0 didn't work" in capsys.readouterr().out
    bad = g["prediction"].copy()
    bad[np.nonzero(g["infinite"] == 0)[0][3], 0] = np.nan                  # the cut refuses non-finite logits
    generate(data, torch.from_numpy(bad).to(DEV), _clf(10.0, "beta"))
    assert "WARNING: Graph cut for 0 didn't work" in capsys.readouterr().out
