"""The exact device graph cut (ops.binary_graph_cut / dgnn_graph_cut_binary, generate_mesh.graph_cut_gpu) against the CPU model of its
contract (tests/graph_cut_model.py): brute force on tiny graphs, scipy's Dinic + residual BFS on larger ones.  Labels bit-equal, energy
and flow value equal."""
import os

import numpy as np
import pytest
import torch

import graph_cut_model as gcm
from dgnn_amd.config import Config
from helpers import gold

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gpu(pred, edges, uw, bw, **kw):
    from dgnn_amd import ops
    out = ops.binary_graph_cut(torch.from_numpy(pred).to(DEV), torch.from_numpy(np.asarray(edges, dtype=np.int32)).to(DEV), uw, bw, **kw)
    assert out[0].is_cuda and out[0].dtype == torch.int32
    return (out[0].cpu().numpy(),) + tuple(out[1:])


def _check(pred, edges, uw, bw, oracle):
    got, e_got, f_got = _gpu(pred, edges, uw, bw)
    D, w = gcm.unary_costs(pred, uw), gcm.potts_weight(bw)
    assert e_got == gcm.energy(got, D, edges, w)
    assert e_got == f_got + int(np.minimum(D[:, 0], D[:, 1]).sum())
    if oracle == "brute":
        want, e_want = gcm.brute_force(pred, edges, uw, bw)
    else:
        want, e_want, f_want = gcm.solve(pred, edges, uw, bw)
        assert f_got == f_want
    assert np.array_equal(got, want) and e_got == e_want


@pytest.mark.parametrize("uw,bw", [(10, 1), (10, 10), (10, 100), (100, 1), (100, 10), (100, 100), (10, 0), (10.0, 10.0)])
def test_tiny_graphs_match_brute_force(uw, bw):
    rng = np.random.default_rng(int(uw) * 1000 + int(bw))
    for trial in range(16):
        n = int(rng.integers(1, 15))
        pred = rng.normal(0, 2, (n, 2)).astype(np.float32)
        if trial % 2 == 0:
            pred[::3, 1] = pred[::3, 0]          # exact ties in the unary cost
            pred[1::4] = 0.0                     # costs of zero
        if trial % 5 == 0:
            pred = -np.abs(pred) - 0.5           # all costs negative
        edges = rng.integers(0, n, (int(rng.integers(0, 3 * n + 1)), 2)).astype(np.int32)   # duplicates, self-loops, isolated cells
        _check(pred, edges, uw, bw, "brute")


def test_tiny_graph_structure_cases():
    pred = np.array([[0.3, 0.1], [0.1, 0.3], [0.2, 0.2], [-1.0, 0.5], [0.0, 0.0], [2.0, -2.0], [0.05, 0.15]], dtype=np.float32)
    for edges in ([], [[0, 1], [0, 1], [1, 1]], [[2, 3], [3, 2], [4, 4], [0, 6]], [[i, j] for i in range(7) for j in range(7)]):
        for bw in (0, 1, 10, 100):
            _check(pred, np.asarray(edges, dtype=np.int32).reshape(-1, 2), 10, bw, "brute")


@pytest.mark.parametrize("n_points", [2000, 20000])
@pytest.mark.parametrize("field", ["noise", "coherent"])
def test_delaunay_graphs_match_dinic(n_points, field):
    edges, cent, nf = gcm.delaunay_facet_graph(n_points, seed=n_points)
    pred = gcm.noise_logits(nf, seed=1) if field == "noise" else gcm.coherent_logits(cent, seed=1)
    for uw, bw in ((10, 1), (10, 10), (100, 10)):
        _check(pred, edges, uw, bw, "dinic")


@pytest.mark.parametrize("bw", [1, 5])
def test_random_graphs_of_high_degree_match_dinic(bw):
    rng = np.random.default_rng(7 + bw)
    n = 5000
    pred = rng.normal(0, 2, (n, 2)).astype(np.float32)
    edges = rng.integers(0, n, (9000 * 3, 2)).astype(np.int32)          # mean degree ~ 11, duplicates and self-loops
    edges[::40, 1] = 17                                                 # one node of degree ~ 700
    _check(pred, edges, 10, bw, "dinic")


@pytest.fixture(scope="module")
def scene_1m():
    edges, cent, nf = gcm.delaunay_facet_graph(150000, seed=0)
    return edges, cent, nf


@pytest.mark.parametrize("field", ["noise", "coherent"])
def test_million_cell_scene_matches_dinic(scene_1m, field):
    edges, cent, nf = scene_1m
    pred = gcm.noise_logits(nf, seed=0) if field == "noise" else gcm.coherent_logits(cent, seed=0)
    _check(pred, edges, 10, 1, "dinic")


def test_million_cell_scene_is_deterministic(scene_1m):
    edges, cent, nf = scene_1m
    pred = gcm.noise_logits(nf, seed=0)
    a = _gpu(pred, edges, 10, 1, return_stats=True)
    b = _gpu(pred, edges, 10, 1, return_stats=True)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_errors_raise():
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    pred = np.random.default_rng(0).normal(0, 1, (6, 2)).astype(np.float32)
    edges = np.array([[0, 1], [2, 3]], dtype=np.int32)
    with pytest.raises(ValueError):
        ops.binary_graph_cut(torch.from_numpy(pred).to(DEV), edges, 10, -1)
    bad = pred.copy()
    bad[3, 1] = np.nan
    with pytest.raises(DgnnError):
        ops.binary_graph_cut(torch.from_numpy(bad).to(DEV), edges, 10, 1)
    with pytest.raises(DgnnError):
        ops.binary_graph_cut(torch.from_numpy(pred).to(DEV), np.array([[0, 6]], dtype=np.int32), 10, 1)
    with pytest.raises(DgnnError):
        ops.binary_graph_cut(torch.from_numpy(pred).to(DEV), np.array([[-1, 2]], dtype=np.int32), 10, 1)
    with pytest.raises(DgnnError):
        ops.binary_graph_cut(torch.from_numpy(pred * 1e9).to(DEV), edges, 10, 1)
    from dgnn_amd.processing.generate_mesh import graph_cut_gpu
    clf = Config(graph_cut=Config(unary_weight=10, binary_weight=1))
    with pytest.raises(ValueError):
        graph_cut_gpu(np.zeros(5, dtype=np.int32), pred, edges, clf)
    # a good call after the failed ones still works
    got, _, _ = _gpu(pred, edges, 10, 1)
    assert np.array_equal(got, gcm.brute_force(pred, edges, 10, 1)[0])


def test_graph_cut_gpu_returns_what_it_was_given():
    from dgnn_amd.processing.generate_mesh import graph_cut_gpu
    rng = np.random.default_rng(4)
    pred = rng.normal(0, 2, (12, 2)).astype(np.float32)
    edges = rng.integers(0, 12, (30, 2)).astype(np.int32)
    clf = Config(graph_cut=Config(unary_weight=10.0, binary_weight=10.0, binary_type=0))
    want = gcm.brute_force(pred, edges, 10.0, 10.0)[0]
    lab = graph_cut_gpu(np.zeros(12, dtype=np.int32), pred, edges, clf)
    assert isinstance(lab, np.ndarray) and np.array_equal(lab, want)
    lab = graph_cut_gpu(torch.zeros(12, dtype=torch.int32, device=DEV), torch.from_numpy(pred).to(DEV), torch.from_numpy(edges), clf)
    assert isinstance(lab, torch.Tensor) and lab.is_cuda and np.array_equal(lab.cpu().numpy(), want)


def _scene(tmp_path):
    g = gold("genmesh_f4_small.npz")
    os.makedirs(os.path.join(str(tmp_path), "gt"), exist_ok=True)
    np.savez(os.path.join(str(tmp_path), "gt", "0_3dt.npz"), vertices=g["vertices"], tetrahedra=g["tetrahedra"], facets=g["facets"], nfacets=g["nfacets"])
    data = Config(path=str(tmp_path), gtfile="gt/0", filename="0", id="", category="", infinite=torch.from_numpy(g["infinite"]))
    return g, data


def _clf(graph_cut, bw, solver="gpu"):
    gc = Config(unary_weight=10.0, binary_weight=bw, binary_type=0)
    if solver is not None:
        gc.solver = solver
    return Config(temp=Config(graph_cut=graph_cut, fix_orientation=0, metrics=[], device=DEV), graph_cut=gc)


@pytest.mark.parametrize("bw", [1.0, 10.0])
def test_generate_with_the_gpu_solver(tmp_path, capsys, bw):
    from dgnn_amd.processing.generate_mesh import generate
    g, data = _scene(tmp_path)
    fin = g["infinite"] == 0
    nf = g["nfacets"]
    edges = nf[(nf >= 0).all(1)]
    want_labels, _, _ = gcm.solve(g["prediction"][fin], edges, 10.0, bw)
    want_faces = gcm.interface_faces(want_labels, nf, g["facets"])
    for pred in (torch.from_numpy(g["prediction"]).to(DEV), torch.from_numpy(g["prediction"])):
        mesh, ev = generate(data, pred, _clf(1, bw))
        assert ev == {} and np.array_equal(np.asarray(mesh.faces), want_faces)
    assert "WARNING" not in capsys.readouterr().out
    if bw == 10.0:     # the cut changes the labels of this scene: the test sees the solver, not the raw arg-max
        assert not np.array_equal(want_faces, g["faces"])
    # graph cut off: the key changes nothing
    mesh, _ = generate(data, torch.from_numpy(g["prediction"]).to(DEV), _clf(0, bw))
    assert np.array_equal(np.asarray(mesh.faces), g["faces"])


def test_generate_falls_back_when_the_gpu_solver_raises(tmp_path, capsys):
    from dgnn_amd.processing.generate_mesh import generate
    g, data = _scene(tmp_path)
    mesh, _ = generate(data, torch.from_numpy(g["prediction"]).to(DEV), _clf(1, -1.0))      # negative weight: ValueError
    assert np.array_equal(np.asarray(mesh.faces), g["faces"])
    assert "WARNING: Graph cut for 0 didn't work" in capsys.readouterr().out
    bad = g["prediction"].copy()
    bad[np.nonzero(g["infinite"] == 0)[0][3], 0] = np.nan
    generate(data, torch.from_numpy(bad).to(DEV), _clf(1, 1.0))
    assert "WARNING: Graph cut for 0 didn't work" in capsys.readouterr().out
