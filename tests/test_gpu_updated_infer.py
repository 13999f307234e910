"""Whole-scene inference of the Updated SurfaceNet on the GPU (surfaceNetUpdatedEdgeFilters.inference_*, csrc/updated_infer.hip) against the fp64 oracle
on the whole-scene adjs of tests/updated_inference_model.py."""
import functools

import numpy as np
import pytest
import torch

from dgnn_amd.config import Config
from dgnn_amd.synthetic import delaunay_tet_graph, hashed_normal
from helpers import gold
from updated_inference_model import make_clf, oracle_net, oracle_whole_scene, whole_scene_adjs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL_LOGIT = 1e-4          # tests/test_gpu_parity.py::test_updated_variant_forward_backward_golden holds this model to it
TOL_ROWS = 2e-6           # the row-level aggregate / GEMM tests of tests/test_gpu_parity.py (rel_err < 2e-6 at the current GEMM mode)
BF = torch.bfloat16
# k_edge_chain_agg (csrc/updated_infer.hip): a workgroup owns TILE_DST consecutive destinations at a time and walks their plan positions
# [rowptr[d0], rowptr[d0 + TILE_DST]) in tiles of TILE_EDGES; a destination's sum is carried from tile to tile
TILE_EDGES, TILE_DST = 64, 16

CASES = {
    "plus": ("sage+", [64, 128, 128, 128], 0b1110),
    "plain": ("sage", [64, 128, 128, 2], 0b1110),
    "fallback": ("sage+", [24, 40, 72, 136], 0),
    "golden": ("sage+", None, None),
}


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def tet_scene():
    adj, _, _ = delaunay_tet_graph(700, seed=7)
    n = adj.shape[0] // 4
    ei = torch.from_numpy(adj.T.astype(np.int64))
    return n, hashed_normal(np.arange(n), 29, seed=1), hashed_normal(np.arange(4 * n), 3, seed=2), ei


@functools.lru_cache(maxsize=None)
def general_scene():
    """N = 64 * 5 + 37 cells, in-degrees from 0 .. 7 with degree-0 rows, self-loops, duplicate edges, shuffled columns (the plan's eid is no identity),
    21 edge columns -- and one segment across every tile boundary of k_edge_chain_agg"""
    n = 64 * 5 + 37
    rng = np.random.default_rng(11)
    deg = rng.integers(0, 8, size=n)
    deg[[0, 5, 17, 100, 200, n - 1]] = 0
    deg[32:48] = 7                                   # 112 positions in one group: a boundary after 64
    deg[160:176] = [7, 7, 7, 7, 7, 7, 7, 7, 7, 1, 0, 7, 7, 7, 7, 7]     # 63 positions, then a 1-edge segment would END at the boundary: fixed up below
    boundaries = []
    for d0 in range(0, n, TILE_DST):
        for _ in range(64):
            start = int(deg[:d0].sum())
            cum = start + np.concatenate([[0], np.cumsum(deg[d0:d0 + TILE_DST])])
            bad = [p for p in range(start + TILE_EDGES, int(cum[-1]), TILE_EDGES) if not any(cum[i] < p < cum[i + 1] for i in range(len(cum) - 1))]
            if not bad:
                break
            i = int(np.nonzero(cum == bad[0])[0][0]) - 1          # the segment that ends at the boundary (or an empty one there)
            while deg[d0 + i] == 0:
                i -= 1
            deg[d0 + i] += 1 if deg[d0 + i] < 7 else -1
        assert not bad
        start, end = int(deg[:d0].sum()), int(deg[:d0 + TILE_DST].sum())
        boundaries += list(range(start + TILE_EDGES, end, TILE_EDGES))
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    assert len(boundaries) >= 3 and int((deg == 0).sum()) >= 5 and deg.max() <= 7
    for p in boundaries:
        assert any(rowptr[d] < p < rowptr[d + 1] for d in range(n))
    dst = np.repeat(np.arange(n), deg)
    src = rng.integers(0, n, size=dst.size)
    src[::9] = dst[::9]                              # self-loops
    src[1::7] = src[0:-1:7][: src[1::7].size]        # duplicate edges where the two positions share a destination (and plain edges elsewhere)
    perm = rng.permutation(dst.size)
    ei = torch.from_numpy(np.stack([src[perm], dst[perm]]).astype(np.int64))
    assert int((ei[0] == ei[1]).sum()) > 0 and np.unique(ei.numpy().T, axis=0).shape[0] < ei.size(1)
    return n, hashed_normal(np.arange(n), 29, seed=3), hashed_normal(np.arange(ei.size(1)), 21, seed=4), ei


@functools.lru_cache(maxsize=None)
def model_case(case):
    """(clf factory, fp32 state dict) of a test model: weights from torch.manual_seed, or the golden ones"""
    name, widths, _ = CASES[case]
    if case == "golden":
        u = gold("updated_f3_blocks.npz")
        widths = [int(v) for v in u["plus.model_params"]]
        sd = {k[len("plus.param."):]: torch.from_numpy(u[k]) for k in u.files if k.startswith("plus.param.")}
    else:
        from oracle.updated_edge_filters import SurfaceNet as Oracle
        torch.manual_seed(sum(widths))
        sd = {k: v.detach().clone() for k, v in Oracle(28, make_clf(widths, name)).state_dict().items()}
    return name, tuple(widths), sd


@functools.lru_cache(maxsize=None)
def reference(case, scene, dtype=torch.float64):
    """the oracle's whole-scene logits, computed once per (model, scene)"""
    name, widths, sd = model_case(case)
    n, x, ea, ei = tet_scene() if scene == "tet" else general_scene()
    net = oracle_net(28, make_clf(widths, name), sd, dtype)
    return oracle_whole_scene(net, x, ea, ei, dtype)


def hip_net(case, dtype=torch.float32, **clf_extra):
    from dgnn_amd.learning.surfaceNetUpdatedEdgeFilters import SurfaceNet
    name, widths, sd = model_case(case)
    clf = make_clf(widths, name, device=DEV)
    for k, v in clf_extra.items():
        clf[k].update(v)
    net = SurfaceNet(28, clf)
    net.load_state_dict(sd)
    return net.to(DEV).eval().set_storage_dtype(dtype)


def scene_data(scene):
    n, x, ea, ei = tet_scene() if scene == "tet" else general_scene()
    return Config(x=x.to(DEV), edge_attr=ea.to(DEV), edge_index=ei.to(DEV))


def spy_on_one_call(monkeypatch):
    """records what ops.updated_infer_fwd reports: the bit mask of the layers that ran through the one-launch form"""
    from dgnn_amd import ops
    seen = []
    real = ops.updated_infer_fwd

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append(out[1])
        return out
    monkeypatch.setattr(ops, "updated_infer_fwd", spy)
    return seen


def check_logits(logits, ref, tol=TOL_LOGIT):
    assert logits.dtype == torch.float32 and tuple(logits.shape) == tuple(ref.shape)
    err = (logits.double().cpu() - ref.double()).abs().max().item()
    bound = tol * max(1.0, ref.abs().max().item())
    print("max|dlogit| %.3e (bound %.3e)" % (err, bound))
    assert err <= bound


# ---- 1. inference_layer against the fp64 oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["plus", "plain", "fallback", "golden"])
def test_inference_layer_matches_the_fp64_oracle(case, monkeypatch):
    seen = spy_on_one_call(monkeypatch)
    logits = hip_net(case).inference_layer(scene_data("tet"))
    check_logits(logits, reference(case, "tet"))
    assert len(seen) == 1
    want = CASES[case][2]
    if want is not None:      # layers 1 - 3 of the 64/128-wide models ran fused (no silent fall-back); no layer of the odd widths did
        assert seen[0] == want


# ---- 2. general CSR ----------------------------------------------------------------------------------------------------------------------------
def test_general_csr_matches_the_fp64_oracle(monkeypatch):
    seen = spy_on_one_call(monkeypatch)
    n, _, ea, ei = general_scene()
    assert n == 64 * 5 + 37 and ea.size(1) == 21
    data = scene_data("general")
    from dgnn_amd.graph import plan_for
    plan = plan_for(data.edge_index, n, n)
    assert not torch.equal(plan.eid.cpu(), torch.arange(plan.E, dtype=torch.int32))
    logits = hip_net("plus").inference_layer(data)
    check_logits(logits, reference("plus", "general"))
    assert seen == [0b1110]


# ---- 3. the per-layer contract of dgnn_edge_chain_aggregate_fwd -------------------------------------------------------------------------
@pytest.mark.parametrize("c_in,k_e", [(64, 28), (128, 64), (128, 128)])
def test_edge_chain_aggregate_layer_contract(c_in, k_e):
    from dgnn_amd import ops
    from oracle.pyg_semantics import propagate_mean
    assert ops.edge_chain_aggregate_supported(c_in, k_e)
    n, _, _, ei = general_scene()
    E = ei.size(1)
    g = torch.Generator().manual_seed(c_in + k_e)
    x = torch.randn(n, c_in, generator=g)
    ea = torch.randn(E, k_e + 4, generator=g)[:, :k_e]                 # row stride k_e + 4
    We, be = torch.randn(c_in, k_e, generator=g) * 0.3, torch.randn(c_in, generator=g)
    phi64 = ea.double() @ We.double().t() + be.double()
    ref_a = propagate_mean(x.double(), n, ei, phi64)
    rowptr, src, eid = ops.plan_build(ei.to(DEV), n, 1)
    ea_dev = torch.empty(E, k_e + 4, device=DEV)
    ea_dev[:, :k_e] = ea.to(DEV)
    args = (rowptr, src, eid, n, x.to(DEV), ea_dev[:, :k_e], We.to(DEV), be.to(DEV))
    a, nxt = ops.edge_chain_aggregate_fwd(*args)
    print("a %.3e  ea_next %.3e" % (rel_err(a, ref_a), rel_err(nxt, torch.relu(phi64))))
    assert rel_err(a, ref_a) < TOL_ROWS
    assert rel_err(nxt, torch.relu(phi64)) < TOL_ROWS
    assert bool((nxt >= 0).all())
    deg = torch.bincount(ei[1], minlength=n)
    assert bool((a[(deg == 0).to(DEV)] == 0).all())
    # write_next = 0: nothing is stored per edge
    poison = torch.full((E, c_in), float("nan"), device=DEV)
    poison[::3] = 7.25
    keep = poison.clone()
    a2, _ = ops.edge_chain_aggregate_fwd(*args, ea_next=poison, write_next=False)
    assert torch.equal(poison.view(torch.int32), keep.view(torch.int32))
    assert torch.equal(a2, a)


# ---- 4. the two block schedules --------------------------------------------------------------------------------------------------------------
def _loader(ei, n, sizes, batch):
    from dgnn_amd.sampler import NeighborSampler
    return NeighborSampler(ei, sizes=sizes, node_idx=None, num_nodes=n, batch_size=batch, shuffle=False)


def _expectation(n, loader):
    """the oracle's rows at every batch's targets, starting from NaN: a row no batch targets stays NaN"""
    expect = torch.full((n, 2), float("nan"), dtype=torch.float64)
    ref = reference("plus", "tet")
    for batch_size, n_id, _ in loader:
        t = n_id[:batch_size].cpu()
        expect[t] = ref[t]
    assert not bool(torch.isnan(expect).any())
    return expect


def test_inference_batch_layer_matches_the_fp64_oracle():
    n, _, _, ei = tet_scene()
    data = scene_data("tet")
    expect = _expectation(n, _loader(data.edge_index, n, [-1] * 4, 256))
    out = hip_net("plus").inference_batch_layer(data, _loader(data.edge_index, n, [-1] * 4, 256))
    check_logits(out, expect)


def test_inference_layer_batch_matches_the_fp64_oracle():
    n, _, _, ei = tet_scene()
    data = scene_data("tet")
    expect = _expectation(n, _loader(data.edge_index, n, [-1], 512))
    out = hip_net("plus").inference_layer_batch(data, _loader(data.edge_index, n, [-1], 512))
    check_logits(out, expect)


# ---- 5. bf16 storage ----------------------------------------------------------------------------------------------------------------------------
def test_bf16_storage_all_three_methods():
    n, x, ea, ei = tet_scene()
    data = scene_data("tet")
    ref = reference("plus", "tet", torch.float32)
    bound = 5e-2 * max(1.0, ref.abs().max().item() / 8)      # tests/test_gpu_bf16.py::test_updated_variant_bf16_forward_backward
    net = hip_net("plus", BF)
    outs = {"inference_layer": net.inference_layer(data),
            "inference_batch_layer": net.inference_batch_layer(data, _loader(data.edge_index, n, [-1] * 4, 256)),
            "inference_layer_batch": net.inference_layer_batch(data, _loader(data.edge_index, n, [-1], 512))}
    for k, out in outs.items():
        assert out.dtype == torch.float32 and tuple(out.shape) == (n, 2)
        err = (out.cpu() - ref).abs().max().item()
        print("%s: max|dlogit| %.3e (bound %.3e)" % (k, err, bound))
        assert err <= bound, k
    # bf16 storage runs on the per-layer kernels forward() runs on: the same bits on whole-scene adjs
    assert net.fused_layers == 0
    with torch.no_grad():
        fwd = net(Config(x=data.x, edge_attr=data.edge_attr, n_id=torch.arange(n, device=DEV),
                         adjs=[(a.to(DEV), e.to(DEV), s) for a, e, s in whole_scene_adjs(ei, n, 4)]))
    assert torch.equal(outs["inference_layer"], fwd)


# ---- 6. Trainer.inference ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_layer,batch_size", [(1, 0), (1, 512), (0, 256)])
def test_trainer_inference_dispatch(per_layer, batch_size):
    from dgnn_amd.learning.runModel import Trainer
    n, x, ea, ei = tet_scene()
    data = scene_data("tet")
    net = hip_net("plus", inference=dict(per_layer=per_layer, has_label=0), temp=dict(batch_size=batch_size))
    clf = net.clf
    mk = lambda: _loader(data.edge_index, n, [-1] if per_layer else [-1] * 4, batch_size) if batch_size else None
    own = {(1, 0): lambda: net.inference_layer(data), (1, 512): lambda: net.inference_layer_batch(data, mk()),
           (0, 256): lambda: net.inference_batch_layer(data, mk())}[(per_layer, batch_size)]()
    out = Trainer(net).inference(data, mk(), clf)
    assert out.device.type == "cpu" and torch.equal(out, own.cpu())
    # with labels: a finite loss and an OA in [0, 100]
    clf.inference.has_label = 1
    clf.regularization.cell_type = "vol"
    clf.regularization.edge_epoch = None
    g = torch.Generator().manual_seed(5)
    occ = torch.rand(n, generator=g)
    data.y = torch.stack([occ, 1 - occ, occ, (occ > 0.5).float()], dim=1).to(DEV)
    data.x = data.x.clone()
    data.x[:, 0] = torch.rand(n, generator=g).to(DEV) + 0.1        # column 0: the cell volumes that weight the loss
    out2 = Trainer(net).inference(data, mk(), clf)
    m = clf.inference.metrics
    assert tuple(out2.shape) == (n, 2) and np.isfinite(float(m.getCellLoss())) and 0.0 <= float(m.getOA()) <= 100.0
