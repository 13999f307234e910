"""normalization 'l' on the GPU: the graph LayerNorm kernels (csrc/lnorm.hip) alone against fp64, and the Static SurfaceNet with LayerNorm
against the reference run (tests/golden/static_ln_*.npz) and the fp64 restatement of layernorm_model.py, in all three inference schedules
and in training."""
import os

import numpy as np
import pytest
import torch

import layernorm_model as R
from dgnn_amd import ops
from dgnn_amd.config import Config, reconbench_pretrained

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


def gold(name):
    return np.load(os.path.join(HERE, "golden", name))


def ln_clf(edge_convs=1, decoder=2, convs=(32, 64, 40)):
    clf = reconbench_pretrained(device=DEV, convs=convs)
    clf.model.normalization = "l"
    clf.model.edge_convs = edge_convs
    clf.model.decoder = decoder
    return clf


# ---- the op alone ------------------------------------------------------------------------------------------------------------------------
def _ref(x, w, b, g, relu, dtype):
    """PyG formula + ReLU on the CPU in `dtype`: (y, dx, dw, db), the gradients of the LayerNorm behind the ReLU for g = dy behind the mask of the
    kernels' own y (an element within rounding of 0 may fall on either side of the ReLU in fp32; the mask is checked through y)"""
    xx = x.detach().cpu().to(dtype).requires_grad_(True)
    ww = w.detach().cpu().to(dtype).requires_grad_(True)
    bb = b.detach().cpu().to(dtype).requires_grad_(True)
    z = R.pyg_layer_norm(xx, ww, bb)
    z.backward(g.cpu().to(dtype))
    y = torch.relu(z) if relu else z
    return [t.detach().double() for t in (y, xx.grad, ww.grad, bb.grad)]


def _check_op(x, relu=True, seed=0):
    M, C = x.shape
    g = torch.Generator().manual_seed(seed)
    w = (1 + 0.3 * torch.randn(C, generator=g)).to(DEV)
    b = (0.2 * torch.randn(C, generator=g)).to(DEV)
    dy = torch.randn(M, C, generator=g).to(DEV)
    y, stats, scale = ops.graph_ln_forward(x, w, b, 1e-5, relu)
    dx, dw, db = ops.graph_ln_relu_bwd(x, dy, stats, w, scale, b, relu)
    g_ = dy * (y > 0) if relu else dy
    ref64 = _ref(x, w, b, g_, relu, torch.float64)
    ref32 = _ref(x, w, b, g_, relu, torch.float32)
    got = [t.double().cpu() for t in (y, dx, dw, db)]
    for k, (gt, r64, r32) in enumerate(zip(got, ref64, ref32)):
        ok = torch.isfinite(r64)      # (a single element: torch's std backward at sigma = 0 is 0 / 0; the kernels return the limit, 0)
        if not bool(ok.any()):
            continue
        e, e32 = (gt - r64)[ok].abs().max().item(), (r32 - r64)[ok].abs().max().item()
        # forward: 4x the error of fp32 torch on the CPU + 1e-6; the gradients are sums over M rows: + 1e-6 of their magnitude
        slack = 1e-6 * (1.0 if k == 0 else max(1.0, r64.abs().max().item()))
        assert e <= 4 * e32 + slack, "%s M=%d C=%d: %.3e vs fp32 CPU %.3e" % (("y", "dx", "dw", "db")[k], M, C, e, e32)
    y2, stats2, scale2 = ops.graph_ln_forward(x, w, b, 1e-5, relu)
    dx2, dw2, db2 = ops.graph_ln_relu_bwd(x, dy, stats2, w, scale2, b, relu)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2), "second run differs"


@pytest.mark.parametrize("M", [1, 7, 1000, 65537])
@pytest.mark.parametrize("C", [1, 3, 40, 64, 128, 256, 1024])
def test_graph_layer_norm_op_against_fp64(M, C):
    g = torch.Generator().manual_seed(M * 31 + C)
    _check_op((0.5 + 2.0 * torch.randn(M, C, generator=g)).to(DEV), seed=M + C)


def test_graph_layer_norm_op_one_million_rows():
    g = torch.Generator().manual_seed(5)
    _check_op(torch.randn(1010078, 128, generator=g).to(DEV), seed=5)


@pytest.mark.parametrize("pad", [4, 5])
def test_graph_layer_norm_op_strided_rows(pad):
    g = torch.Generator().manual_seed(pad)
    big = torch.randn(3001, 64 + pad, generator=g).to(DEV)
    _check_op(big[:, :64], seed=pad)
    _check_op(big[:, :64], relu=False, seed=pad)


def test_graph_layer_norm_op_offset_and_constant_and_empty():
    g = torch.Generator().manual_seed(9)
    _check_op((1e3 + torch.randn(4099, 40, generator=g)).to(DEV), seed=9)       # offset by 1e3 sigma
    x = torch.full((513, 24), 2.5, device=DEV)
    w, b = torch.rand(24, device=DEV) + 0.5, torch.randn(24, device=DEV)
    y = ops.graph_ln_forward(x, w, b, 1e-5, False)[0]
    assert torch.equal(y, b.expand(513, 24))                                     # 0 / (0 + eps) * w + b
    e = torch.empty((0, 16), device=DEV)
    y, st, sc = ops.graph_ln_forward(e, w[:16], b[:16], 1e-5, True)
    assert y.shape == (0, 16)
    dx, dw, db = ops.graph_ln_relu_bwd(e, e, st, w[:16], sc, b[:16], True)
    assert dx.shape == (0, 16) and torch.equal(dw, torch.zeros(16, device=DEV)) and torch.equal(db, torch.zeros(16, device=DEV))


@pytest.mark.parametrize("M,n_out", [(1000, 64), (65537, 128), (65537, 256), (7, 40)])
def test_gemm_epilogue_and_standalone_statistics(M, n_out):
    """relu(LN(A1 W1^T + A2 W2^T + b)) with the statistics from the GEMM epilogue (where dgnn_linear_fwd_x3_stats takes the shape) and from the
    standalone pass over the same product: both against fp64"""
    g = torch.Generator().manual_seed(M + n_out)
    A1, A2 = torch.randn(M, 48, generator=g), torch.randn(M, 32, generator=g)
    W1, W2 = torch.randn(n_out, 48, generator=g) / 7, torch.randn(n_out, 32, generator=g) / 6
    bias, w, b = torch.randn(n_out, generator=g), 1 + 0.3 * torch.randn(n_out, generator=g), 0.2 * torch.randn(n_out, generator=g)
    z64 = A1.double() @ W1.double().t() + A2.double() @ W2.double().t() + bias.double()
    y64 = torch.relu(R.pyg_layer_norm(z64, w.double(), b.double()))
    d = [t.to(DEV) for t in (A1, W1, A2, W2, bias, w, b)]
    y, z, _, _ = ops.linear_fwd_ln(*d, eps=1e-5, relu=True)
    assert (y.double().cpu() - y64).abs().max().item() <= 1e-4 * max(1.0, y64.abs().max().item())
    zz = ops.linear_fwd(d[0], d[1], d[2], d[3], d[4])
    y2 = ops.graph_ln_forward(zz, d[5], d[6], 1e-5, True)[0]
    assert (y2.double().cpu() - y64).abs().max().item() <= 1e-4 * max(1.0, y64.abs().max().item())
    y3 = ops.linear_fwd_ln(*d, eps=1e-5, relu=True)[0]
    assert torch.equal(y, y3)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def _scene():
    s = gold("static_ln_scene.npz")
    x, ea = torch.from_numpy(s["x"]), torch.from_numpy(s["edge_attr"])
    ei = torch.from_numpy(s["adjacencies"].T.astype(np.int64))
    adjs = [(torch.from_numpy(s["adj%d_edge_index" % i]), torch.from_numpy(s["adj%d_e_id" % i]), tuple(int(v) for v in s["adj%d_size" % i]))
            for i in range(3)]
    return x, ea, ei, torch.from_numpy(s["n_id"]), adjs


def _net(edge_convs, decoder=2, sd=None, seed=0):
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import LayerNorm, SurfaceNet
    torch.manual_seed(seed)
    net = SurfaceNet(ln_clf(edge_convs, decoder))
    if sd is not None:
        net.load_state_dict(sd)
    else:
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, LayerNorm):
                    m.weight.copy_(1 + 0.3 * torch.randn(m.weight.shape))
                    m.bias.copy_(0.2 * torch.randn(m.bias.shape))
    return net.to(DEV)


def _close_logits(got, ref):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape
    bound = 1e-4 * ref.abs().clamp(min=1.0)
    assert bool(((got - ref).abs() <= bound).all()), "max |dlogit| %.3e" % (got - ref).abs().max().item()
    if ref.size(1) == 2:
        clear = (ref[:, 0] - ref[:, 1]).abs() > 1e-3
        assert torch.equal(got.argmax(1)[clear], ref.argmax(1)[clear])


def _cases():
    out = []
    for e in (1, 2):
        g = gold("static_ln_e%d.npz" % e)
        out.append((e, 2, {k[len("param."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param.")}, g))
    for e in (1, 2):
        out.append((e, 1, None, None))
    return out


@pytest.mark.parametrize("case", range(4))
def test_model_inference_layer_and_training_step_against_reference(case):
    e, dec, sd, g = _cases()[case]
    net = _net(e, dec, sd, seed=case)
    p = R.params64({k: v.cpu() for k, v in net.state_dict().items()}, requires_grad=True)
    x, ea, ei, n_id, adjs = _scene()
    net.eval()
    lg = net.inference_layer(Config(x=x.to(DEV), edge_attr=ea.to(DEV), edge_index=ei.to(DEV)))
    with torch.no_grad():
        lg64 = R.inference_layer(p, x.double(), ea.double(), ei)
    _close_logits(lg, lg64)
    if g is not None:
        _close_logits(lg, g["logits"])
        assert (lg64 - torch.from_numpy(g["logits64"])).abs().max().item() <= 1e-10
    # train forward + backward on the 3-hop blocks: the autograd path (the whole-model and direct-step forms decline LayerNorm)
    net.train()
    data = Config(all=Config(x=x.to(DEV), edge_attr=ea.to(DEV)), batch_n_id=n_id.to(DEV), batch_adjs=[(a.to(DEV), e_.to(DEV), s) for a, e_, s in adjs])
    assert net._train_spec(x.to(DEV), data, DEV) is None
    tl = net(data)
    tl64 = R.forward_blocks(p, x.double(), ea.double(), n_id, adjs)
    _close_logits(tl, tl64.detach())
    G = torch.from_numpy(g["G"]) if g is not None else torch.randn(tl.shape, generator=torch.Generator().manual_seed(case))
    if g is not None:
        _close_logits(tl, g["train_logits"])
    (tl * G.to(DEV)).sum().backward()
    (tl64 * G.double()).sum().backward()
    for k, t in net.named_parameters():
        ref = p[k].grad
        err = (t.grad.double().cpu() - ref).norm().item()
        assert err <= 1e-4 * max(ref.norm().item(), 1e-6), "%s: |dgrad| %.3e vs |grad| %.3e" % (k, err, ref.norm().item())
        if g is not None:
            assert np.linalg.norm(t.grad.double().cpu().numpy() - g["grad." + k]) <= 1e-4 * max(np.linalg.norm(g["grad." + k]), 1e-6), k


def _loaders(n, ei_np, hops):
    from oracle.pyg_semantics import neighbor_sampler_full
    bl, lb = [], []
    for s in range(0, n, 150):
        batch = np.arange(s, min(n, s + 150))
        n_id, adjs = neighbor_sampler_full(ei_np, n, batch, hops)
        bl.append((len(batch), torch.from_numpy(n_id), [(torch.from_numpy(a), torch.from_numpy(e), sz) for a, e, sz in adjs]))
        n_id, adjs = neighbor_sampler_full(ei_np, n, batch, 1)
        a, e, sz = adjs[0]
        lb.append((len(batch), torch.from_numpy(n_id), (torch.from_numpy(a), torch.from_numpy(e), sz)))
    return bl, lb


@pytest.mark.parametrize("edge_convs", [1, 2])
def test_schedules_follow_the_reference_loops(edge_convs):
    """inference_batch_layer / inference_layer_batch normalise per batch (and the layer-major decoder over the scene), as the reference's loops do:
    they match the per-batch fp64 restatement and differ from inference_layer by more than the tolerance"""
    g = gold("static_ln_e%d.npz" % edge_convs)
    sd = {k[len("param."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param.")}
    net = _net(edge_convs, 2, sd).eval()
    p = R.params64({k: v for k, v in sd.items()})
    x, ea, ei, _, _ = _scene()
    n = x.size(0)
    bl, lb = _loaders(n, ei.numpy(), 3)
    assert len(bl) >= 3
    whole = net.inference_layer(Config(x=x.to(DEV), edge_attr=ea.to(DEV), edge_index=ei.to(DEV)))
    dev_bl = [(bs, nid.to(DEV), [(a.to(DEV), e.to(DEV), s) for a, e, s in adjs]) for bs, nid, adjs in bl]
    dev_lb = [(bs, nid.to(DEV), (a.to(DEV), e.to(DEV), s)) for bs, nid, (a, e, s) in lb]
    got_bl = net.inference_batch_layer(Config(x=x.to(DEV), edge_attr=ea.to(DEV)), dev_bl)
    got_lb = net.inference_layer_batch(Config(x=x.to(DEV), edge_attr=ea.to(DEV)), dev_lb)
    with torch.no_grad():
        ref_bl = R.inference_batch_layer(p, x.double(), ea.double(), bl)
        ref_lb = R.inference_layer_batch(p, x.double(), ea.double(), lb)
    _close_logits(got_bl, ref_bl)
    _close_logits(got_lb, ref_lb)
    for got in (got_bl, got_lb):
        assert (got - whole).abs().max().item() > 1e-2, "the schedule made no difference"


def test_trainer_adam_steps_follow_the_fp64_restatement():
    from dgnn_amd.learning.runModel import Metrics, Trainer
    from oracle.pyg_semantics import neighbor_sampler_full
    x, ea, ei, _, _ = _scene()
    n = x.size(0)
    occ = torch.sigmoid(2 * x[:, 3:4] + x[:, 7:8])
    y = torch.cat([occ, 1 - occ], 1)
    net = _net(2, 2, None, seed=7).train()
    clf = net.clf
    clf.training.metrics = Metrics()
    clf.temp.current_epoch = 0
    p = R.params64({k: v.cpu() for k, v in net.state_dict().items()}, requires_grad=True)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    opt64 = torch.optim.Adam([p[k] for k, _ in net.named_parameters()], lr=1e-3)
    tr = Trainer(net)
    for step in range(5):
        batch = np.arange(40 * step, 40 * step + 32)
        n_id, adjs = neighbor_sampler_full(ei.numpy(), n, batch, 3)
        adjs = [(torch.from_numpy(a), torch.from_numpy(e), s) for a, e, s in adjs]
        n_id = torch.from_numpy(n_id)
        data = Config(all=Config(x=x.to(DEV), y=y.to(DEV), edge_attr=ea.to(DEV)), batch_n_id=n_id.to(DEV),
                      batch_adjs=[(a.to(DEV), e.to(DEV), s) for a, e, s in adjs])
        loss = tr.train(data, opt, clf).item()
        lg = R.forward_blocks(p, x.double(), ea.double(), n_id, adjs)
        tgt = n_id[:len(batch)]
        vol = x[tgt, 0].double()
        cell = torch.nn.functional.kl_div(torch.log_softmax(lg, -1), y[tgt].double(), reduction="none").sum(1) * vol
        loss64 = cell.sum() / vol.sum()
        opt64.zero_grad()
        loss64.backward()
        opt64.step()
        assert abs(loss - loss64.item()) <= 1e-4 * abs(loss64.item()), "step %d: %.8f vs %.8f" % (step, loss, loss64.item())


def test_guards_bf16_storage_and_partitioned_scene():
    from dgnn_amd.partition import PartitionedScene
    net = _net(1).eval()
    with pytest.raises(NotImplementedError):
        net.set_storage_dtype(torch.bfloat16)
    scene = PartitionedScene.build_synthetic(300, 3, 0, 1, DEV)
    with pytest.raises(NotImplementedError):
        scene.inference_layer(net)
