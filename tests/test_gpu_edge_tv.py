"""The edge total-variation regulariser on the device (csrc/edge_tv.hip -> ops.edge_tv_* -> functional.edge_tv -> Trainer) against its fp64 model
(tests/edge_tv_model.py, held to the reference-run values by tests/test_edge_tv_model_cpu.py) and against the values the reference's own
learning/runModel.py produced (tests/golden/trainer_f2.npz).  Tolerances: 3e-6 relative on values, 3e-6 * max|grad| on gradients -- what
tests/test_reference_host_cpu.py holds the same quantities to; bit equality between the direct step, the autograd path and reruns."""
import functools
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import edge_tv_model as M
from dgnn_amd.config import Config, reconbench_pretrained
from helpers import gold
from test_gpu_parity import DEV, hip_static
from test_reference_host_cpu import loss_clf
from test_trainer_cpu import make_clf

pytestmark = pytest.mark.gpu

W = 0.37
TOL = 3e-6
Adj = namedtuple("Adj", ["edge_index", "e_id", "size"])


@functools.lru_cache(maxsize=None)
def case(name):
    """(logits, edge_index, model at g = 1.7) of one shape, computed once and left unchanged"""
    logits, ei, ties = M.make_case(name)
    M.assert_separated(logits, ei, ties)          # the condition on the inputs: must hold, not a reason to skip
    return logits, ei, M.edge_tv(logits, ei, W, g=1.7)


def layout(ei, dtype, kind):
    """edge_index on the device as a whole [2, E] tensor, as a column slice of a wider one (rows with a storage offset, not 16-byte aligned) or as
    the transposed view of an [E, 2] array (what the scene loader hands out)"""
    t = torch.from_numpy(ei).to(dtype)
    if kind == "whole":
        return t.to(DEV)
    if kind == "slice":
        pad = torch.full((2, 1), -7, dtype=dtype)
        big = torch.cat([pad, t, pad, pad], 1).to(DEV)
        out = big[:, 1:1 + t.size(1)]
        assert out.data_ptr() % 16 != 0 and out.storage_offset() == 1
        return out
    return t.t().contiguous().to(DEV).t()


def check_against_model(m, reg, sums, dl, E):
    print("reg %.9g model %.9g | reg_sum %.12g model %.12g | max|dgrad| %.3g of %.3g" % (
        reg.item(), m["reg"], sums[0].item(), m["reg_sum"], np.abs(dl.double().cpu().numpy() - m["dlogits"]).max(), np.abs(m["dlogits"]).max()))
    assert reg.dtype == torch.float32 and sums.dtype == torch.float64 and sums.shape == (2,)
    assert abs(reg.item() - m["reg"]) <= TOL * m["reg"]
    assert abs(sums[0].item() - m["reg_sum"]) <= TOL * m["reg_sum"]
    assert sums[1].item() == E
    assert np.abs(dl.double().cpu().numpy() - m["dlogits"]).max() <= TOL * np.abs(m["dlogits"]).max()


@pytest.mark.parametrize("kind", ["whole", "slice", "pairs"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("name", M.CASES)
def test_ops_match_the_model(name, dtype, kind):
    from dgnn_amd import ops
    logits, ei, m = case(name)
    lg, e = torch.from_numpy(logits).to(DEV), layout(ei, dtype, kind)
    E, g = ei.shape[1], torch.tensor(1.7, device=DEV)
    if name == "large_aligned" and kind == "whole":
        assert e.data_ptr() % 16 == 0 and e[1].data_ptr() % 16 == 0          # the two-row 16-byte form, int32 and int64
    for max_blocks in ((None, 3) if name.startswith("large") else (None,)):      # 3 workgroups: several passes of the grid whatever the index form
        reg, sums, net = ops.edge_tv_fwd(lg, e, W, max_blocks=max_blocks)
        dl = ops.edge_tv_bwd(lg, net, W, E, g)
        check_against_model(m, reg, sums, dl, E)
        if name == "self_loop":
            assert reg.item() == 0 and not dl.any()
        assert np.array_equal(net.cpu().numpy(), m["c"])          # the integer counts are exact, node 123 of the large cases (5 000 atomics) included
        if name == "tiny":
            assert not dl[4].any()
        # forward without a gradient, and the two-launch step (written, and added into an existing gradient): the same bits
        reg0, sums0, none = ops.edge_tv_fwd(lg, e, W, need_grad=False, max_blocks=max_blocks)
        assert none is None and torch.equal(reg0, reg) and torch.equal(sums0, sums)
        running = torch.tensor([2.0, 5.0], dtype=torch.float64, device=DEV)
        base = torch.full((logits.shape[0], 2), 0.25, device=DEV)
        loss = torch.tensor(0.5, device=DEV)
        reg1, sums1, dl1, total = ops.edge_tv_step(lg, e, W, grad_loss=g, add_loss=loss, running=running, dlogits=base.clone(), max_blocks=max_blocks)
        assert torch.equal(reg1, reg) and torch.equal(sums1, sums) and torch.equal(dl1, base + dl) and torch.equal(total, loss + reg)
        assert torch.equal(running, torch.tensor([2.0, 5.0], dtype=torch.float64, device=DEV) + sums)
        reg2, sums2, dl2, none = ops.edge_tv_step(lg, e, W, grad_loss=g, max_blocks=max_blocks)      # (the kept count table came back zeroed)
        assert none is None and torch.equal(reg2, reg) and torch.equal(dl2, dl)
        assert ops._tv_net and not any(t.any() for t in ops._tv_net.values())


def test_saturated_rows_are_finite_with_zero_gradient():
    from dgnn_amd import ops
    logits = np.array([[200.0, 0.0], [0.0, 200.0], [0.5, -0.5], [-300.0, 300.0], [2.0, 0.0]], np.float32)
    ei = np.array([[0, 1, 3, 4], [1, 2, 0, 1]], np.int64)
    m = M.edge_tv(logits, ei, W)
    reg, sums, dl, _ = ops.edge_tv_step(torch.from_numpy(logits).to(DEV), torch.from_numpy(ei).to(DEV), W)
    assert torch.isfinite(reg) and torch.isfinite(sums).all() and torch.isfinite(dl).all()
    assert not dl[[0, 1, 3]].any()          # exp(-200) is 0 in fp32: p (1 - p) = 0 exactly
    assert dl[2, 0] > 0 and dl[4, 0] > 0          # (the rows in between keep theirs)
    check_against_model(m, reg, sums, dl, 4)


@pytest.mark.parametrize("name", ["remainders", "large", "large_aligned"])
def test_reruns_are_bit_identical(name):
    from dgnn_amd import ops
    logits, ei, _ = case(name)
    lg, e = torch.from_numpy(logits).to(DEV), torch.from_numpy(ei).to(DEV)
    a = ops.edge_tv_step(lg, e, W)
    b = ops.edge_tv_step(lg, e, W)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    x = lg.clone().requires_grad_(True)
    from dgnn_amd import functional as Fn
    reg, sums = Fn.edge_tv(x, e, W)
    reg.backward()
    assert torch.equal(reg.detach(), a[0]) and torch.equal(sums, a[1]) and torch.equal(x.grad, a[2])      # autograd path: the same bits


def test_argument_checks():
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    lg, e = torch.zeros(4, 2, device=DEV), torch.zeros((2, 3), dtype=torch.int64, device=DEV)
    for bad_l, bad_e, err in ((lg.cpu(), e, DgnnError), (lg.double(), e, TypeError), (torch.zeros(4, 3, device=DEV), e, ValueError), (lg, e.cpu(), DgnnError),
                              (lg, e.float(), TypeError), (lg, e[:, :0], ValueError), (lg, e[0], ValueError)):
        with pytest.raises(err):
            ops.edge_tv_fwd(bad_l, bad_e, W)
        with pytest.raises(err):
            ops.edge_tv_step(bad_l, bad_e, W)


class Spy:
    """counts the calls of ops.edge_tv_fwd / _bwd / _step"""

    def __init__(self, monkeypatch):
        from dgnn_amd import ops
        self.calls = {}
        for name in ("edge_tv_fwd", "edge_tv_bwd", "edge_tv_step"):
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def wrapped(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a, **k)
        return wrapped

    def take(self):
        calls, self.calls = self.calls, {}
        return calls


def fixture_data(g, dev):
    gt, bx = torch.from_numpy(g["batch_gt"]).to(dev), torch.from_numpy(g["batch_x"]).to(dev)
    adjs = [Adj(None, None, (0, 0))] * 4 + [Adj(torch.from_numpy(g["reg_edge_index"]).to(dev), None, (int(g["reg_n_inner"]), 40))]
    return (("batch", Config(batch_gt=gt, batch_x=bx, batch_adjs=adjs)),
            ("whole", Config(batch_gt=gt, batch_x=bx, batch_adjs=[], edge_index=torch.from_numpy(g["reg_whole_edge_index"]).to(dev))))


def test_trainer_takes_the_device_path_on_the_reference_fixture(monkeypatch):
    from dgnn_amd.learning import runModel as R
    g = gold("trainer_f2.npz")
    spy = Spy(monkeypatch)
    tr = R.Trainer(Config(num_layers=4))
    for tag, data in fixture_data(g, DEV):
        clf = loss_clf("kl", None, DEV, edge_epoch=2, epoch=3, hops=1)
        logits = torch.from_numpy(g["reg_logits"]).to(DEV).requires_grad_(True)
        m = R.Metrics()
        total = tr.calcLossAndOA(logits, None, data, clf, m)
        total.backward()
        assert spy.take() == {"edge_tv_fwd": 1, "edge_tv_bwd": 1}, tag
        want, gw = float(g["total_" + tag]), torch.from_numpy(g["total_grad_" + tag])
        rs, es, rl = g["reg_metrics_" + tag]
        print(tag, total.item(), want, (logits.grad.cpu() - gw).abs().max().item(), gw.abs().max().item(), m.reg_sum, rs)
        assert abs(total.item() - want) <= TOL * want
        assert (logits.grad.cpu() - gw).abs().max().item() <= TOL * gw.abs().max().item()
        assert m.edges_sum == es and abs(m.reg_sum - rs) <= TOL * rs and abs(m.getRegLoss() - rl) <= TOL * rl
        clf.temp.current_epoch = 1          # before regularization.edge_epoch: cell loss only, no regulariser launch
        early = tr.calcLossAndOA(logits.detach(), None, data, clf, R.Metrics())
        assert spy.take() == {} and abs(early.item() - float(g["total_early_" + tag])) <= TOL * float(g["total_early_" + tag])


def test_fallbacks_keep_the_torch_chain(monkeypatch):
    """CPU logits, fp64 logits, no edges and DGNN_FUSED_LOSS=0: the reference's op chain, value for value, and no library call"""
    from dgnn_amd.learning import runModel as R
    g = gold("trainer_f2.npz")
    spy = Spy(monkeypatch)
    tr = R.Trainer(Config(num_layers=4))
    clf = loss_clf("kl", None, DEV, edge_epoch=2, epoch=3, hops=1)

    def chain(logits, ei):
        inner = torch.softmax(logits, dim=-1)
        tv = torch.abs(inner[ei[0, :]][:, 0] - inner[ei[1, :]][:, 0]) * clf.regularization.edge_weight
        return tv.mean(), tv.sum()

    for dev, dtype, fused, edges in (("cpu", torch.float32, True, True), (DEV, torch.float64, True, True), (DEV, torch.float32, True, False),
                                     (DEV, torch.float32, False, True)):
        monkeypatch.setattr(R, "FUSED_KL_LOSS", fused)
        for tag, data in fixture_data(g, dev):
            logits = torch.from_numpy(g["reg_logits"]).to(dev).to(dtype)
            if not edges:
                if tag == "batch":
                    data.batch_adjs[4] = Adj(data.batch_adjs[4].edge_index[:, :0], None, data.batch_adjs[4].size)
                else:
                    data.edge_index = data.edge_index[:, :0]
            m = R.Metrics()
            reg = tr.calcRegularization(logits, data, clf, m)
            ei = data.batch_adjs[4].edge_index if tag == "batch" else data.edge_index
            want, want_sum = chain(logits[:int(g["reg_n_inner"])] if tag == "batch" else logits, ei)
            assert spy.take() == {}, (dev, dtype, fused, edges, tag)
            assert reg.dtype == dtype and (torch.equal(reg, want) if edges else bool(torch.isnan(reg)))
            assert m.edges_sum == ei.size(1) and m.reg_sum == want_sum.item()


@functools.lru_cache(maxsize=None)
def small_scene():
    """tests/golden/scene_small through the scene loader: x [n, 29], edge_attr [4n, 20], edge_index (the transposed view of its [E, 2] array), y"""
    from dgnn_amd.processing.data import dataLoader
    clf = reconbench_pretrained()
    clf.temp.cell_order = "none"
    dl = dataLoader(clf, verbosity=0)
    root = os.path.join(os.path.dirname(__file__), "golden", "scene_small")
    dl.run(dict(path=root, filename="0", category="", id="", scan_conf="", gtfile="gt/0", ioufile=""))
    return Config(x=dl.features, edge_attr=dl.edge_features, edge_index=dl.edge_lists, y=dl.gt.float(), infinite=dl.infinite)


def test_direct_step_with_the_regulariser(monkeypatch):
    """Trainer._train_direct with an active regulariser on 5-hop blocks (num_hops 4 + 1): bit-identical to the autograd path over functional.edge_tv,
    and within the reference tolerances of the torch chain (DGNN_FUSED_LOSS=0)."""
    from dgnn_amd.learning import runModel as R
    from dgnn_amd.sampler import NeighborSampler
    sc = small_scene()
    n = sc.x.size(0)
    ei = sc.edge_index.contiguous()
    spy = Spy(monkeypatch)
    out = {}
    for mode in ("direct", "autograd", "torch"):
        monkeypatch.setattr(R, "TRAIN_DIRECT", mode == "direct")
        monkeypatch.setattr(R, "FUSED_KL_LOSS", mode != "torch")
        clf = make_clf()
        clf.temp.device, clf.temp.current_epoch, clf.regularization.edge_epoch = DEV, 3, 2
        clf.training.metrics = R.Metrics()
        net = hip_static(train=True)
        tr, opt = R.Trainer(net), R.make_adam(net.parameters(), 0.005)
        _, n_id, adjs = NeighborSampler(ei, sizes=[-1] * 5, num_nodes=n, batch_size=12, prefetch=False).sample(torch.arange(40, 52, device=DEV))
        assert len(adjs) == 5 and adjs[4].edge_index.size(1) > 0 and adjs[4].size[0] == adjs[3].size[1]
        d = Config(all=sc, batch_n_id=n_id, batch_adjs=adjs)
        if mode == "direct":
            loss = tr._train_direct(d, opt, clf, None)
            assert loss is not None          # (None on the parent: an active regulariser sent the step to the autograd engine)
            assert spy.take() == {"edge_tv_step": 1}
        else:
            loss = tr.train(d, opt, clf)
            assert spy.take() == ({"edge_tv_fwd": 1, "edge_tv_bwd": 1} if mode == "autograd" else {})
        m = clf.training.metrics
        out[mode] = (loss.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters()},
                     (m.reg_sum, m.edges_sum, m.cell_sum, m.weight_sum, m.OA_sum, m.samples_sum))
        assert m.edges_sum == adjs[4].edge_index.size(1) and m.reg_sum > 0
    assert torch.equal(out["direct"][0], out["autograd"][0]) and out["direct"][2] == out["autograd"][2]
    for k, v in out["autograd"][1].items():
        assert torch.equal(out["direct"][1][k], v), k
    want = out["torch"][0].item()
    print("loss", out["direct"][0].item(), want)
    assert abs(out["direct"][0].item() - want) <= TOL * abs(want)
    # gradients against the torch chain: 2e-4 of the largest entry, what test_trainer_train_steps_hip_model_match_the_reference_run applies to a training
    # step against the reference on the F3 blocks.  The biases ahead of a train-mode BatchNorm have an analytically zero gradient and both sides
    # hold rounding noise: they get the absolute 1e-9 that test_gpu_train._same_grad gives the same keys.
    for k, v in out["torch"][1].items():
        err, scale = (out["direct"][1][k] - v).abs().max().item(), v.abs().max().item()
        print(k, err, scale)
        if k.endswith("lin_j.bias") or k == "decoder.0.bias":
            assert err <= 1e-9, (k, err)
        else:
            assert err <= 2e-4 * scale, (k, err, scale)


def test_additional_hops_config_error_still_exits():
    from dgnn_amd.learning import runModel as R
    from dgnn_amd.sampler import NeighborSampler
    sc = small_scene()
    clf = make_clf()
    clf.temp.device, clf.temp.current_epoch, clf.regularization.edge_epoch, clf.graph.additional_num_hops = DEV, 3, 2, 0
    clf.training.metrics = R.Metrics()
    net = hip_static(train=True)
    _, n_id, adjs = NeighborSampler(sc.edge_index.contiguous(), sizes=[-1] * 4, num_nodes=sc.x.size(0), batch_size=12, prefetch=False).sample(
        torch.arange(40, 52, device=DEV))
    with pytest.raises(SystemExit):
        R.Trainer(net).train(Config(all=sc, batch_n_id=n_id, batch_adjs=adjs), R.make_adam(net.parameters(), 0.005), clf)


def test_validation_takes_the_whole_graph_branch_on_the_device(monkeypatch):
    from dgnn_amd.learning import runModel as R
    sc = small_scene()
    spy = Spy(monkeypatch)
    clf = make_clf()
    clf.temp.device, clf.temp.current_epoch, clf.regularization.edge_epoch, clf.temp.batch_size = DEV, 3, 2, 0
    assert clf.inference.has_label and clf.inference.per_layer
    logits = R.Trainer(hip_static()).inference(Config(x=sc.x, edge_attr=sc.edge_attr, edge_index=sc.edge_index, y=sc.y, infinite=sc.infinite), [], clf)
    assert spy.take() == {"edge_tv_fwd": 1} and not logits.is_cuda
    m = M.edge_tv(logits.numpy(), sc.edge_index.cpu().numpy(), clf.regularization.edge_weight)
    im = clf.inference.metrics
    print(im.reg_sum, m["reg_sum"], im.edges_sum, m["edges"])
    assert im.edges_sum == m["edges"] and abs(im.reg_sum - m["reg_sum"]) <= TOL * m["reg_sum"]
    assert abs(im.getRegLoss() - m["reg"]) <= TOL * m["reg"]
