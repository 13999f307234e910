"""Sampled neighbourhoods in the GPU k-hop block builder (NeighborSampler sizes[h] > 0): the builder against the numpy model of
tests/sampled_blocks_model.py, exactly, on every path that builds blocks; and the consumers -- Static and Updated model, Trainer -- on
sampled blocks against the CPU oracle run on the same blocks."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sampled_blocks_model as M
from dgnn_amd.config import Config
from helpers import oracle_static
from test_gpu_parity import DEV, TOL_LOGIT, hip_static
from test_trainer_cpu import make_clf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 37, 128)
FULL = [-1] * 3     # the full-neighbourhood instantiation of the builder's kernels, on both graphs
REG_SIZES = ([2] * 4, [3, 1, 2], [-1, 2, -1, 3], FULL)
IRR_SIZES = REG_SIZES + ([5] * 2,)
CASES = [(name, sizes, nb) for name, sl in (("regular", REG_SIZES), ("irregular", IRR_SIZES)) for sizes, nb in itertools.product(sl, BATCHES)]
CASES.sort(key=lambda c: c[1] is FULL)      # (stable) the FULL cases last: a case's id carries its position, and the earlier cases keep theirs


@pytest.fixture(scope="module")
def graphs():
    out = {}
    for name, (ei, n) in (("regular", M.regular_graph()), ("irregular", M.irregular_graph())):
        out[name] = (ei, n, torch.from_numpy(ei).to(DEV))
    return out


@pytest.fixture(scope="module")
def scene(graphs):
    """the regular graph with 28 + 1 node features (column 0 = the cell volume), 20 edge features, occupancy labels"""
    from dgnn_amd.synthetic import hashed_normal
    ei, n, ei_dev = graphs["regular"]
    x = hashed_normal(np.arange(n), 29, seed=1, device=DEV)
    x[:, 0] = x[:, 0].abs() + 0.05
    ea = hashed_normal(np.arange(4 * n), 20, seed=2, device=DEV)
    occ = torch.sigmoid(2 * x[:, 3:4] + x[:, 7:8])
    return Config(x=x, y=torch.cat([occ, 1 - occ], 1), edge_attr=ea, n=n, ei=ei_dev)


def _sampler(graphs, name, sizes, **kw):
    from dgnn_amd.sampler import NeighborSampler
    ei, n, ei_dev = graphs[name]
    return NeighborSampler(ei_dev, sizes=sizes, num_nodes=n, **kw)


def _adjs(adjs):
    return [adjs] if isinstance(adjs[0], torch.Tensor) else list(adjs)


def _snapshot(block):
    """a block as numpy arrays (buffer-ring blocks are only valid until two more have been drawn)"""
    from dgnn_amd.graph import plan_for
    bs, n_id, adjs = block
    return bs, n_id.cpu().numpy().copy(), [(e.cpu().numpy().copy(), i.cpu().numpy().copy(), tuple(int(v) for v in s),
                                            plan_for(e, s[0], s[1]).rowptr.cpu().numpy().astype(np.int64)) for e, i, s in _adjs(adjs)]


def _same_blocks(a, b):
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and len(a[2]) == len(b[2])
    for (e1, i1, s1, o1), (e2, i2, s2, o2) in zip(a[2], b[2]):
        assert s1 == s2 and np.array_equal(e1, e2) and np.array_equal(i1, i2) and np.array_equal(o1, o2)


def _batch(graphs, name, nb):
    ei, n, _ = graphs[name]
    batch = np.random.default_rng(100 + nb).permutation(n)[:nb].astype(np.int64)
    if name == "irregular" and nb > 1:
        deg = np.bincount(ei[1], minlength=n)
        head = np.asarray([int(np.nonzero(deg == d)[0][0]) for d in (0, 12, 9)], dtype=np.int64)      # the degree classes are in the batch itself, not only behind it
        batch = np.concatenate([head, batch[~np.isin(batch, head)]])[:nb]      # (nb - 3 others: the permutation prefix holds at least nb - 3 of them)
        assert batch.size == nb and len(set(batch.tolist())) == nb
    return batch


# ---- 1. the builder equals the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sizes,nb", CASES)
def test_builder_equals_the_model(graphs, name, sizes, nb):
    """n_id, both rows of every edge_index, every e_id, every size and the row offsets, integer-exact, for two seeds x two draws (the regular graph
    takes the one-call builder, the irregular one -- in-degrees 0..12: nothing to draw, the register path, the loop path -- the hop-by-hop one);
    sizes [-1] * 3 hold the full-neighbourhood instantiation of the kernels to the model on both paths"""
    ei, n, _ = graphs[name]
    batch = _batch(graphs, name, nb)
    for seed, draw in itertools.product((0, 0xD1B54A32D192ED03), (0, 5)):
        loader = _sampler(graphs, name, sizes, batch_size=nb, prefetch=False, sample_seed=seed)
        got = _snapshot(loader.sample(torch.from_numpy(batch).to(DEV), draw=draw))
        assert loader.draws == 0        # a pinned draw is not counted
        ref_n_id, ref = M.sampled_blocks(ei, n, batch, sizes, seed, draw, with_off=True)
        assert got[0] == nb and np.array_equal(got[1], ref_n_id) and len(got[2]) == len(sizes)
        for (e, e_id, size, off), (re, reid, rsize, roff) in zip(got[2], ref):
            assert size == tuple(rsize)
            assert np.array_equal(e[0], re[0]) and np.array_equal(e[1], re[1]) and np.array_equal(e_id, reid) and np.array_equal(off, roff)


# ---- 2. every path agrees ----------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
import numpy as np
import torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import sampled_blocks_model as M
import dgnn_amd.sampler as S
assert not S.ONE_CALL
ei, n = M.regular_graph()
idx = torch.from_numpy(np.random.default_rng(1).permutation(n)[:537].astype(np.int64)).to("cuda:0")
out = {}
for tag, prefetch in (("inline", False), ("side", True)):
    loader = S.NeighborSampler(torch.from_numpy(ei).to("cuda:0"), sizes=[2, 3, 2], node_idx=idx, num_nodes=n, batch_size=100, prefetch=prefetch, sample_seed=77)
    for k, (bs, n_id, adjs) in enumerate(loader):
        out["%s.%d.n_id" % (tag, k)] = n_id.cpu().numpy()
        for h, (e, i, s) in enumerate(adjs):
            out["%s.%d.%d.e" % (tag, k, h)], out["%s.%d.%d.i" % (tag, k, h)] = e.cpu().numpy(), i.cpu().numpy()
    assert loader.draws == 6
torch.cuda.synchronize()
np.savez(sys.argv[2], **out)
"""


def test_every_path_builds_the_same_blocks(graphs, tmp_path):
    """in-line, side stream, worker thread and the library thread with the buffer ring, over 5 batches of 100 targets and a ragged sixth: identical
    blocks, with draw numbers in batch order; the transposed plans that come with the block equal dgnn_plan_build by source; and the hop-by-hop
    builder (DGNN_KHOP_ONE_CALL=0, a fresh process) builds them too"""
    from dgnn_amd import ops
    from dgnn_amd.graph import plan_for
    ei, n, _ = graphs["regular"]
    idx = torch.from_numpy(np.random.default_rng(1).permutation(n)[:537].astype(np.int64)).to(DEV)
    sizes = [2, 3, 2]

    def run(**kw):
        loader = _sampler(graphs, "regular", sizes, node_idx=idx, batch_size=100, sample_seed=77, **kw)
        out = []
        for block in loader:
            assert loader.draws == len(out) + 1
            if kw.get("prefetch", True):
                for e, i, s in _adjs(block[2]):
                    plan = plan_for(e, s[0], s[1])
                    assert plan._t is not None and plan.has_edge_rows          # came with the block
                    t_ref = ops.plan_build(e, s[0], by=0, hint=ops.PLAN_HINT_GENERIC, n_other=s[1])
                    for a, b in zip(plan.transposed, t_ref):
                        assert torch.equal(a, b)
                    assert torch.equal(plan.edge_rows.long(), i) and torch.equal(plan.transposed_edge_rows.long(), i[t_ref[2].long()])
            out.append(_snapshot(block))
        assert len(out) == 6 and out[-1][0] == 37 and loader.draws == 6
        return out
    ref = run(prefetch=False)
    for k, blk in enumerate(ref):           # ... which are the model's blocks with draw = batch number
        rn, radjs = M.sampled_blocks(ei, n, idx[k * 100:(k + 1) * 100].cpu().numpy(), sizes, 77, k, with_off=True)
        _same_blocks(blk, (blk[0], rn, [(e, i, tuple(s), o) for e, i, s, o in radjs]))
    for kw in (dict(prefetch=True), dict(prefetch="thread"), dict(prefetch=True, reuse_buffers=True)):
        for a, b in zip(ref, run(**kw)):
            _same_blocks(a, b)
    # a second pass continues the count: draws 6..11, other blocks than the first pass
    loader = _sampler(graphs, "regular", sizes, node_idx=idx, batch_size=100, sample_seed=77, reuse_buffers=True)
    first = [_snapshot(b) for b in loader]
    second = [_snapshot(b) for b in loader]
    assert loader.draws == 12
    _same_blocks(first[0], ref[0])
    rn, radjs = M.sampled_blocks(ei, n, idx[:100].cpu().numpy(), sizes, 77, 6, with_off=True)
    _same_blocks(second[0], (100, rn, [(e, i, tuple(s), o) for e, i, s, o in radjs]))
    # the hop-by-hop builder on the same regular graph, in a fresh process
    script, out = tmp_path / "child.py", tmp_path / "blocks.npz"
    script.write_text(_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], cwd=ROOT, env=dict(os.environ, DGNN_KHOP_ONE_CALL="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    got = np.load(str(out))
    for tag in ("inline", "side"):
        for k, blk in enumerate(ref):
            assert np.array_equal(got["%s.%d.n_id" % (tag, k)], blk[1])
            for h, (e, i, s, o) in enumerate(blk[2]):
                assert np.array_equal(got["%s.%d.%d.e" % (tag, k, h)], e) and np.array_equal(got["%s.%d.%d.i" % (tag, k, h)], i)


# ---- 3. sizes that drop nothing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sizes", [("regular", [4, 7, 4]), ("regular", [5, -1, 4, 4]), ("irregular", [12, 12]), ("irregular", [40, -1, 12])])
@pytest.mark.parametrize("kw", [dict(prefetch=False), dict(prefetch=True), dict(prefetch=True, reuse_buffers=True)], ids=["inline", "side", "ring"])
def test_sizes_at_or_above_the_in_degree_give_the_full_blocks(graphs, name, sizes, kw):
    ei, n, _ = graphs[name]
    idx = torch.arange(0, 300, device=DEV)
    a = [_snapshot(b) for b in _sampler(graphs, name, sizes, node_idx=idx, batch_size=128, sample_seed=3, **kw)]
    b = [_snapshot(b) for b in _sampler(graphs, name, [-1] * len(sizes), node_idx=idx, batch_size=128, **kw)]
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        _same_blocks(x, y)


# ---- 4. the rows gathered behind sampled blocks ------------------------------------------------------------------------------------------
def test_attach_rows_on_sampled_blocks(scene, graphs):
    import dgnn_amd.sampler as SM
    from dgnn_amd.sampler import block_rows
    loader = _sampler(graphs, "regular", [2] * 4, node_idx=torch.arange(0, 437, device=DEV), batch_size=100, reuse_buffers=True, sample_seed=5)
    loader.attach_rows([(scene.x, 1, 28, "all"), (scene.x, 0, 29, "batch"), (scene.y, 0, 2, "batch")])
    seen = 0
    for bs, n_id, adjs in loader:
        assert adjs[0].size[0] == n_id.numel()
        for src, c0, nc, which in ((scene.x, 1, 28, "all"), (scene.x, 0, 29, "batch"), (scene.y, 0, 2, "batch")):
            got = block_rows(n_id, src, c0, nc, which)
            assert (got is not None) == SM.ONE_CALL
            if got is not None:
                ids = n_id if which == "all" else n_id[:bs]
                assert torch.equal(got, src[ids, c0:c0 + nc]), (which, c0)
        seen += 1
    assert seen == 5


# ---- 5. the Static model on sampled blocks -----------------------------------------------------------------------------------------------
def _cpu_blocks(n_id, adjs):
    return n_id.cpu(), [(e.cpu().clone(), i.cpu().clone(), tuple(int(v) for v in s)) for e, i, s in _adjs(adjs)]


def test_static_model_on_sampled_blocks_matches_the_oracle(scene, graphs):
    """widths [64, 128, 128, 128], 28 node / 20 edge features, sizes [2] * 4, 128 targets: train-mode logits, running statistics and every parameter
    gradient against oracle/static_edge_filters.py on the same blocks, with the bounds of the same comparison on full blocks
    (tests/test_gpu_parity.py::test_train_forward_backward_golden_f3, restated); eval-mode inference_batch_layer and inference_layer_batch within
    the fp32 logit bound"""
    batch = torch.from_numpy(np.random.default_rng(8).permutation(scene.n)[:128].astype(np.int64)).to(DEV)
    loader = _sampler(graphs, "regular", [2] * 4, batch_size=128, prefetch=False, sample_seed=11)
    bs, n_id, adjs = loader.sample(batch, draw=2)
    assert [a.edge_index.size(1) for a in adjs] == [2 * a.size[1] for a in adjs] and adjs[-1].size[1] == 128
    c_n_id, c_adjs = _cpu_blocks(n_id, adjs)
    x, ea = scene.x.cpu(), scene.edge_attr.cpu()
    G = torch.from_numpy(np.random.default_rng(2).standard_normal((128, 2)).astype(np.float32))
    onet = oracle_static(train=True)
    ol = onet(Config(all=Config(x=x, edge_attr=ea), batch_n_id=c_n_id, batch_adjs=c_adjs))
    (ol * G).sum().backward()
    net = hip_static(train=True)
    logits = net(Config(all=Config(x=scene.x, edge_attr=scene.edge_attr), batch_n_id=n_id, batch_adjs=adjs))
    err = (logits.detach().cpu() - ol.detach()).abs().max().item()
    print("train logits", err)
    assert err <= TOL_LOGIT
    (logits * G.to(DEV)).sum().backward()
    og = dict(onet.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in og.values())
    for k, p in net.named_parameters():
        ref = og[k].grad
        err = (p.grad.cpu() - ref).abs().max().item()
        assert err <= 2e-4 * ref.abs().max().item() + 2e-6 * gmax, (k, err, ref.abs().max().item(), gmax)
    ob = dict(onet.named_buffers())
    for k, b in net.named_buffers():
        ref = ob[k].double()
        err = (b.cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
        assert err < 1e-5, (k, err)
    # eval mode: batch-major on sampled 4-hop blocks, layer-major on sampled 1-hop blocks
    net, onet = hip_static(), oracle_static()
    idx = torch.arange(0, 237, device=DEV)
    data_all, odata = Config(x=scene.x, edge_attr=scene.edge_attr), Config(x=x, edge_attr=ea)
    with torch.no_grad():
        for sizes, sched, node_idx, bsz in (([2] * 4, "inference_batch_layer", idx, 100), ([2], "inference_layer_batch", torch.arange(0, scene.n, device=DEV), 512)):
            blocks = list(_sampler(graphs, "regular", sizes, node_idx=node_idx, batch_size=bsz, sample_seed=4))      # (fresh tensors per block: they keep)
            cpu_blocks = []
            for bs, n_id, adjs in blocks:
                c_n_id, c_adjs = _cpu_blocks(n_id, adjs)
                cpu_blocks.append((bs, c_n_id, c_adjs if len(sizes) > 1 else c_adjs[0]))
            got = getattr(net, sched)(data_all, blocks)
            want = getattr(onet, sched)(odata, cpu_blocks)
            sel = node_idx.cpu()
            err = (got.cpu()[sel] - want[sel]).abs().max().item()
            print(sched, err)
            assert err <= TOL_LOGIT


def test_static_direct_step_equals_the_autograd_step_on_sampled_blocks(scene, graphs):
    """three Trainer.train steps over a sampled loader: the direct step (no autograd engine) and the autograd path, bit for bit -- losses, parameters,
    BatchNorm buffers, the last step's gradients"""
    import dgnn_amd.learning.runModel as RM
    from dgnn_amd.learning.runModel import Metrics, Trainer
    out = {}
    for direct in (True, False):
        RM.TRAIN_DIRECT = direct
        try:
            clf = make_clf()
            clf.temp.device, clf.temp.current_epoch = DEV, 0
            clf.training.metrics = Metrics()
            net = hip_static(train=True)
            tr, opt = Trainer(net), RM.make_adam(net.parameters(), 0.005)
            loader = _sampler(graphs, "regular", [2] * 4, node_idx=torch.arange(0, 3 * 128, device=DEV), batch_size=128, sample_seed=21)
            losses = [tr.train(Config(all=scene, batch_n_id=n_id, batch_adjs=adjs), opt, clf).item() for bs, n_id, adjs in loader]
            out[direct] = (losses, {k: v.detach().clone() for k, v in net.state_dict().items()}, {k: p.grad.clone() for k, p in net.named_parameters()})
        finally:
            RM.TRAIN_DIRECT = True
    assert len(out[True][0]) == 3 and out[True][0] == out[False][0]
    for part in (1, 2):
        for k in out[False][part]:
            assert torch.equal(out[True][part][k], out[False][part][k]), k


# ---- 6. the Updated model on sampled blocks ----------------------------------------------------------------------------------------------
def test_updated_model_on_sampled_blocks_matches_the_oracle(scene, graphs, monkeypatch):
    """widths [64, 128, 128, 128], "+" head, sizes [2] * 4: logits, every layer's phi at the block's e_id and every gradient against
    oracle/updated_edge_filters.py on the same blocks (bounds of tests/test_gpu_parity.py::test_updated_variant_forward_backward_golden).  Hops
    draw independently, so an inner block holds edges that the block outside it lacks: their phi rows read as zeros, as the reference's zeroed
    [E_all, C] tensor gives them -- the input is checked to contain such edges."""
    from dgnn_amd import functional as Fn
    from dgnn_amd import ops
    from dgnn_amd.learning.surfaceNetUpdatedEdgeFilters import SurfaceNet as Updated
    from oracle.updated_edge_filters import SurfaceNet as OracleUpdated
    batch = torch.from_numpy(np.random.default_rng(8).permutation(scene.n)[:128].astype(np.int64)).to(DEV)
    bs, n_id, adjs = _sampler(graphs, "regular", [2] * 4, batch_size=128, prefetch=False, sample_seed=11).sample(batch, draw=1)
    absent = [int((~torch.isin(inner.e_id, outer.e_id)).sum().item()) for outer, inner in zip(adjs[:-1], adjs[1:])]
    print("edges of a block that the block outside it lacks:", absent)
    assert min(absent) > 0
    c_n_id, c_adjs = _cpu_blocks(n_id, adjs)
    x, ea = scene.x.cpu(), scene.edge_attr.cpu()
    G = torch.from_numpy(np.random.default_rng(2).standard_normal((128, 2)).astype(np.float32))
    cfg = lambda dev: Config.wrap(dict(training=dict(model_params=[64, 128, 128, 128], model_name="sage+", loss="kl"),
                                       features=dict(normalization_feature=1, keep_normalization_feature=0), temp=dict(device=dev)))
    torch.manual_seed(3)
    onet = OracleUpdated(28, cfg("cpu"))
    odata = Config(x=x, edge_attr=ea, n_id=c_n_id, adjs=c_adjs)
    trace = []
    with torch.no_grad():
        ref = onet(odata, trace=trace)
    ref_phi = [t for k, t in trace if k.startswith("phi")]
    # the oracle's "+" head applies an in-place ReLU to a ReLU's output and cannot run backward; the same function with the head's modules applied
    # out of place (relu(relu(x)) = relu(x)) gives the same logits bit for bit and the reference gradients
    plain = OracleUpdated(28, Config.wrap(dict(training=dict(model_params=[64, 128, 128, 128], model_name="sage", loss="kl"),
                                               features=dict(normalization_feature=1, keep_normalization_feature=0), temp=dict(device="cpu"))))
    plain.convs = onet.convs
    h = torch.relu(plain(odata))
    ol = onet.out_net[3](torch.relu(onet.out_net[1](h)))
    assert torch.equal(ol.detach(), ref)
    (ol * G).sum().backward()

    phis = []
    real_stack, real_layer = ops.updated_stack_fwd, Fn.sage_updated_layer

    def stack(x0, edge_attr_all, pos, layers):
        y, saved = real_stack(x0, edge_attr_all, pos, layers)
        buf, offs, widths = saved[0], saved[1], saved[2]
        phis[:] = [torch.as_strided(buf.view(torch.float32), (l["plan"].E, widths[i]), (widths[i], 1), offs[i]["phi"] // 4).clone() for i, l in enumerate(layers)]
        return y, saved

    def layer(*a, **k):
        out = real_layer(*a, **k)
        phis.append(out[1].detach().clone())
        return out
    monkeypatch.setattr(ops, "updated_stack_fwd", stack)
    monkeypatch.setattr(Fn, "sage_updated_layer", layer)
    net = Updated(28, cfg(DEV))
    net.load_state_dict(onet.state_dict())
    net = net.to(DEV).train()
    logits = net(Config(x=scene.x, edge_attr=scene.edge_attr, n_id=n_id, adjs=adjs))
    err = (logits.detach().cpu() - ref).abs().max().item()
    print("logits", err, ref.abs().max().item())
    assert err <= TOL_LOGIT * max(1.0, ref.abs().max().item())
    assert len(phis) == 4
    for i, (phi, want) in enumerate(zip(phis, ref_phi)):
        want = want[c_adjs[i][1]]
        err = (phi.cpu() - want).abs().max().item()
        print("phi", i, err, want.abs().max().item())
        assert phi.shape == want.shape and err <= TOL_LOGIT * max(1.0, want.abs().max().item())
    (logits * G.to(DEV)).sum().backward()
    og = dict(onet.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in og.values())
    grads = {}
    for k, p in net.named_parameters():
        r = og[k].grad
        err = (p.grad.cpu() - r).abs().max().item()
        assert err <= 2e-4 * r.abs().max().item() + 2e-6 * gmax, (k, err, r.abs().max().item())
        grads[k] = p.grad.clone()
    # the direct step on the same blocks: the autograd path's gradients, bit for bit (when this configuration takes the one-call form)
    loss = net.train_step_direct(Config(x=scene.x, edge_attr=scene.edge_attr, n_id=n_id, adjs=adjs), lambda lg: ((lg * G.to(DEV)).sum(), G.to(DEV)))
    if loss is not None:
        for k, p in net.named_parameters():
            assert torch.equal(p.grad, grads[k]), k


# ---- 7. the Trainer ----------------------------------------------------------------------------------------------------------------------
def test_trainer_steps_from_the_buffer_ring_equal_the_in_line_loader(scene, graphs):
    """three Trainer.train steps (kl loss, the edge regulariser on the extra hop's block) from a buffer-ring loader with sizes [2] * 5 and from a
    prefetch=False loader: losses and final parameters bit for bit"""
    import dgnn_amd.learning.runModel as RM
    from dgnn_amd.learning.runModel import Metrics, Trainer
    out = []
    for kw in (dict(prefetch=False), dict(prefetch=True, reuse_buffers=True)):
        clf = make_clf()
        clf.temp.device, clf.temp.current_epoch, clf.regularization.edge_epoch, clf.graph.additional_num_hops = DEV, 3, 2, 1
        assert clf.training.loss == "kl"
        clf.training.metrics = Metrics()
        net = hip_static(train=True)
        tr, opt = Trainer(net), RM.make_adam(net.parameters(), 0.005)
        loader = _sampler(graphs, "regular", [2] * 5, node_idx=torch.arange(0, 3 * 128, device=DEV), batch_size=128, sample_seed=9, **kw)
        if "reuse_buffers" in kw:
            tr.attach_block_rows(loader, scene, net)
        losses = []
        for bs, n_id, adjs in loader:
            assert len(adjs) == 5 and adjs[4].size == (adjs[3].size[1], 128) and adjs[4].edge_index.size(1) == 256
            losses.append(tr.train(Config(all=scene, batch_n_id=n_id, batch_adjs=adjs), opt, clf))
        torch.cuda.synchronize()
        assert clf.training.metrics.edges_sum == 3 * 256         # the regulariser ran, on the innermost (extra hop's) block
        out.append((torch.stack(losses).cpu(), {k: v.detach().clone() for k, v in net.state_dict().items()}))
    assert out[0][0].numel() == 3 and torch.equal(out[0][0], out[1][0])
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k


# ---- 8. the constructor ------------------------------------------------------------------------------------------------------------------
def test_constructor_checks_sizes_and_full_sizes_keep_the_existing_entry_points(graphs, monkeypatch):
    import dgnn_amd.sampler as SM
    for bad in ([2, 0, 2], [-2], [3, -2]):
        with pytest.raises(ValueError):
            _sampler(graphs, "regular", bad, batch_size=8)
    called = []
    real = SM.lib()

    class Spy:
        def __getattr__(self, name):
            if name.startswith("dgnn_khop"):
                called.append(name)
            return getattr(real, name)
    monkeypatch.setattr(SM, "lib", lambda: Spy())
    batch = torch.arange(50, 90, device=DEV)
    for name in ("regular", "irregular"):
        full = _sampler(graphs, name, [-1] * 4, batch_size=40, prefetch=False, sample_seed=123)
        a = _snapshot(full.sample(batch, draw=0))
        b = _snapshot(full.sample(batch, draw=9))
        c = _snapshot(full.sample(batch))
        assert full.draws == 1
        _same_blocks(a, b), _same_blocks(a, c)
    assert called and not [c for c in called if "sampled" in c], called
    del called[:]
    _sampler(graphs, "regular", [2] * 4, batch_size=40, prefetch=False).sample(batch)
    _sampler(graphs, "irregular", [2] * 4, batch_size=40, prefetch=False).sample(batch)
    assert [c for c in called if "sampled" in c]


# ---- 9. size = -1 through the _sampled per-hop entry points ------------------------------------------------------------------------------
def test_sampled_entry_points_with_size_minus_one_build_the_full_blocks(graphs, monkeypatch):
    """include/dgnn_hip.h: dgnn_khop_count_sampled / dgnn_khop_expand_sampled with size = -1 give the result of the plain entry points, whatever
    the seed and the draw.  Two hops on the irregular graph, 37 targets with in-degrees 0, 12 and 9 among them: the loader's calls of the plain
    entry points are redirected to the _sampled ones with (size -1, a seed, a draw, hop 0), the blocks equal the un-redirected loader's"""
    import dgnn_amd.sampler as SM
    batch = torch.from_numpy(_batch(graphs, "irregular", 37)).to(DEV)
    want = _snapshot(_sampler(graphs, "irregular", [-1] * 2, batch_size=37, prefetch=False).sample(batch))
    called = []
    real = SM.lib()
    split = {"dgnn_khop_count": 4, "dgnn_khop_expand": 7}       # the _sampled forms take (size, seed, draw, hop) after this many arguments

    class Spy:
        def __getattr__(self, name):
            if name not in split:
                return getattr(real, name)
            called.append(name)
            k = split[name]
            return lambda *a: getattr(real, name + "_sampled")(*a[:k], -1, 0x9E3779B97F4A7C15, 3, 0, *a[k:])
    monkeypatch.setattr(SM, "lib", lambda: Spy())
    got = _snapshot(_sampler(graphs, "irregular", [-1] * 2, batch_size=37, prefetch=False).sample(batch))
    assert called == ["dgnn_khop_count", "dgnn_khop_expand"] * 2
    _same_blocks(got, want)


# ---- 10. a capacity that is too small ----------------------------------------------------------------------------------------------------
def test_a_capacity_too_small_at_hop_1_leaves_the_builder_clean(graphs):
    """the one-call builder with cap_t[1] = 1, sizes [2, 3, 2], 37 targets: DGNN_E_INVALID that names the hop and the capacity, after hop 0 has been
    committed -- and `pos` / `first` are as between batches, so the next block is the model's"""
    from dgnn_amd._lib import DgnnError
    ei, n, _ = graphs["regular"]
    sizes = [2, 3, 2]
    batch = _batch(graphs, "regular", 37)
    loader = _sampler(graphs, "regular", sizes, batch_size=37, prefetch=False, sample_seed=77)
    with torch.cuda.device(loader.device):
        b = loader._alloc_regular(37, True)
        cap_t = b["args_tail"][6]
        assert list(cap_t) == [37, 37 * 3, 37 * 3 * 4]
        cap_t[1] = 1
        with pytest.raises(DgnnError, match=r"hop 1 needs \d+ targets / \d+ edges, capacity 1 / "):
            loader._start_regular(torch.from_numpy(batch).to(DEV), background=False, b=b)
    assert bool((loader._pos == -1).all().item()) and bool((loader._first == 2 ** 31 - 1).all().item())
    rn, radjs = M.sampled_blocks(ei, n, batch, sizes, 77, 0, with_off=True)
    _same_blocks(_snapshot(loader.sample(torch.from_numpy(batch).to(DEV), draw=0)), (37, rn, [(e, i, tuple(s), o) for e, i, s, o in radjs]))
