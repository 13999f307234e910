"""CPU model of the bf16 STORAGE path's error: the oracle's fp32 arithmetic with the activations ROUNDED where the HIP path
stores them -- after conv -> norm -> relu of every layer that is written to HBM, in the format it is written in (bf16: 8 significant bits; the
unsigned rows of round 4: 9).  The compensated arithmetic of csrc/fused_bf16.hip leaves nothing else, so this model predicts the GPU's max / rms
|dlogit| and arg-max agreement to three digits (tests/test_gpu_bf16.py prints the GPU's; `python tests/test_bf16_rounding_model_cpu.py 150000`
prints the model's table for the 1M-tet metric graph: ~15 s per row on 8 cores).  Test infrastructure: imports the oracle."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def round_bits(h, drop):
    """keep 24 - drop significant bits of non-negative fp32 values, round to nearest even (drop = 16: bf16; 15: the unsigned 16-bit rows)"""
    b = h.contiguous().view(torch.int32)
    half = (1 << (drop - 1)) - 1
    return ((b + half + ((b >> drop) & 1)) >> drop << drop).view(torch.float32)


def run(net, x, ea, ei, store_drop, own_drop=(0, 0, 0, 0)):
    """store_drop[i]: bits dropped where layer i's output is stored (0 = not stored / fp32); own_drop[i]: additional rounding of layer i+1's OWN-row
    operand (the unsigned own row goes to the matrix cores as bf16)"""
    h = x[:, 1:]
    hs = hd = h
    with torch.no_grad():
        for i in range(4):
            h = net.convs[i][2](net.convs[i][1](net.convs[i][0]((hs, hd), ea, ei)))
            hs = round_bits(h, store_drop[i]) if store_drop[i] else h
            hd = round_bits(hs, own_drop[i]) if own_drop[i] else hs
        return net.decoder(hs)


ROWS = (("round 3: four layers bf16, decoder apart", (16, 16, 16, 16), (0, 0, 0, 0)),
        ("decoder in the last launch: three layers bf16", (16, 16, 16, 0), (0, 0, 0, 0)),
        ("unsigned rows, own row as (hi, lo)", (15, 15, 15, 0), (0, 0, 0, 0)),
        ("unsigned rows, own row rounded to bf16 (shipped)", (15, 15, 15, 0), (16, 16, 16, 0)))


def table(points, threads=8):
    import bench
    from helpers import oracle_static
    torch.set_num_threads(threads)
    adj, _, x, ea = bench.make_scene(points, 0)
    ei = torch.from_numpy(adj.T.astype(np.int64))
    net = oracle_static()
    ref = run(net, x, ea, ei, (0, 0, 0, 0))
    out = []
    for name, sd, od in ROWS:
        e = (run(net, x, ea, ei, sd, od) - ref).abs()
        g = run(net, x, ea, ei, sd, od)
        out.append((name, e.max().item(), e.pow(2).mean().sqrt().item(), (g.argmax(1) == ref.argmax(1)).float().mean().item()))
    return out


def test_rounding_helper_is_round_to_nearest_even():
    v = torch.tensor([1.0, 1.0 + 2 ** -8, 1.0 + 2 ** -9, 1.0 + 3 * 2 ** -9, 3.0e5, 1e-20, 0.0])
    assert torch.equal(round_bits(v, 16), v.to(torch.bfloat16).float())                         # bf16 of non-negative values
    got = round_bits(v, 15)
    assert got[1] == v[1] and got[2] == 1.0 and got[3] == 1.0 + 2 ** -7 and got[6] == 0.0      # 9 significant bits, ties to even


def test_storage_format_ordering_on_a_small_scene():
    """130k tets: each step of BASELINE.md's table shrinks the error as on the metric graph (decoder in the launch < four bf16 layers; unsigned rows ~ half)"""
    rows = table(20000, threads=min(os.cpu_count() or 8, 8))
    rms = [r[2] for r in rows]
    assert rms[1] < 0.9 * rms[0] and rms[2] < 0.6 * rms[1] and rms[2] < rms[3] < 0.75 * rms[1], rms
    assert rows[3][1] < 5e-2 and rows[3][3] > 0.999, rows[3]


if __name__ == "__main__" and not (len(sys.argv) > 2 and sys.argv[2] == "train"):
    for name, mx, rms, agree in table(int(sys.argv[1]) if len(sys.argv) > 1 else 150000):
        print("%-52s max %.3e  rms %.3e  arg-max agreement %.5f" % (name, mx, rms, agree))


# ---- training twin (tests/bf16_training_model.py): the Updated variant's step with the bf16 roundings of the HIP path injected ---------------------------
def _updated_block(points, batch, params, seed=1):
    """a sampled 4-hop block of a small Delaunay scene for the Updated model (CPU sampler restated in oracle/pyg_semantics.py), random-init weights"""
    from dgnn_amd.config import Config
    from dgnn_amd.synthetic import delaunay_tet_graph
    from oracle.pyg_semantics import neighbor_sampler_full
    from oracle.updated_edge_filters import SurfaceNet as ONet
    adj, _, _ = delaunay_tet_graph(points, seed)
    n = adj.shape[0] // 4
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 29, generator=g)
    ea = torch.randn(4 * n, 20, generator=g)
    idx = torch.randperm(n, generator=g)[:batch].numpy()
    n_id, adjs = neighbor_sampler_full(adj.T.astype(np.int64), n, idx, len(params))
    adjs = [(torch.from_numpy(a), torch.from_numpy(e), s) for a, e, s in adjs]
    G = torch.randn(batch, params[-1], generator=g)
    clf = Config.wrap(dict(training=dict(model_params=list(params), model_name="sage", loss="kl"),
                           features=dict(normalization_feature=1, keep_normalization_feature=0), temp=dict(device="cpu")))
    torch.manual_seed(5)
    net = ONet(28, clf)
    return net, x, ea, torch.from_numpy(n_id), adjs, G, clf


def test_training_model_without_rounding_is_the_oracle():
    """every rounding site off: the explicit forward / backward of tests/bf16_training_model.py == the oracle's autograd step in fp64 (this pins the model)"""
    from bf16_training_model import error_table, updated_step
    from dgnn_amd.config import Config
    params = (16, 24, 32, 8)
    net, x, ea, n_id, adjs, G, _ = _updated_block(400, 24, params)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)      # the oracle's torch.zeros([E_all, C]) (reference :236)
    try:
        onet = net.double()
        ologits = onet(Config(x=x.double(), edge_attr=ea.double(), n_id=n_id, adjs=adjs))
        (ologits * G.double()).sum().backward()
    finally:
        torch.set_default_dtype(old)
    logits, grads = updated_step(net.state_dict(), params, 28, x, ea, n_id, adjs, G, sites=())
    assert (logits - ologits.detach()).abs().max().item() <= 1e-12 * max(1.0, ologits.abs().max().item())
    ref = {k: p.grad for k, p in onet.named_parameters()}
    assert set(ref) == set(grads)
    for k, (mx, rms) in error_table(ref, grads).items():
        assert mx <= 1e-11, (k, mx)


def training_price_table(points, batch, params, threads=8):
    """[(sites switched on, {param: (max err / max, rms err / rms)})]: the un-rounded step against the model with all sites, and with one family of
    sites left in fp32 at a time -- which stored tensor the gradient error of bf16 storage comes from."""
    from bf16_training_model import ALL_SITES, error_table, updated_step
    torch.set_num_threads(threads)
    net, x, ea, n_id, adjs, G, _ = _updated_block(points, batch, params)
    sd = net.state_dict()
    _, ref = updated_step(sd, params, 28, x, ea, n_id, adjs, G, sites=())
    rows = []
    for name, sites in (("all sites (the HIP path)", ALL_SITES), ("weights kept fp32 in the products", ALL_SITES - {"w"}), ("dy / da / dx kept fp32", ALL_SITES - {"dy"}),
                        ("dphi / d_ea kept fp32", ALL_SITES - {"dphi"}), ("dy and dphi kept fp32 (forward storage only)", ALL_SITES - {"dy", "dphi"}),
                        ("forward tensors kept fp32 (backward storage only)", frozenset({"dy", "dphi"}))):
        _, got = updated_step(sd, params, 28, x, ea, n_id, adjs, G, sites=sites)
        rows.append((name, error_table(ref, got)))
    return rows


def test_training_model_rounding_sites_add_up_on_a_small_block():
    """the model with all sites differs from the un-rounded step at bf16 level (a few 1e-3 .. 1e-1 of a gradient tensor), and leaving a family of
    sites in fp32 never makes the worst layer WORSE by more than noise -- the table BASELINE.md section 4 quotes is made by this function"""
    rows = training_price_table(600, 32, (32, 48, 64, 16), threads=min(os.cpu_count() or 8, 8))
    worst = {name: max(v[1] for v in tab.values()) for name, tab in rows}
    full = worst["all sites (the HIP path)"]
    assert 1e-4 < full < 0.5, worst
    assert worst["dy and dphi kept fp32 (forward storage only)"] <= full * 1.2 and worst["forward tensors kept fp32 (backward storage only)"] <= full * 1.2, worst


if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[2] == "train":
    # python tests/test_bf16_rounding_model_cpu.py 10000 train [w0,w1,w2,w3] [batch]: the price table of the training step (rms error / rms gradient per conv layer)
    params = tuple(int(v) for v in (sys.argv[3] if len(sys.argv) > 3 else "128,256,512,1024").split(","))
    for name, tab in training_price_table(int(sys.argv[1]), int(sys.argv[4]) if len(sys.argv) > 4 else 1024, params):
        print(name)
        for l in range(len(params)):
            print("   layer %d: " % l + "  ".join("%s rms %.2e max %.2e" % (k.split(".", 2)[2], tab[k][1], tab[k][0]) for k in sorted(tab) if k.startswith("convs.%d." % l)))


# ---- Static twin (tests/bf16_training_model.py::static_step): the main model's bf16 training step ------------------------------------------------------
def _static_block(points, batch, convs, seed=1, shipped=False):
    """a sampled 4-hop block of a small Delaunay scene for the Static model (CPU sampler restated in oracle/pyg_semantics.py): x [n, 29] (column 0
    is dropped by regularization.cell_type), edge rows [4n, 20], target-gradient G; the kf96 weights at the shipped widths, else random-init weights
    with BatchNorm affine parameters and running buffers drawn away from their init -> (fp64 oracle net, x, ea, n_id, adjs, G)"""
    from dgnn_amd.synthetic import delaunay_tet_graph
    from helpers import oracle_static
    from oracle.pyg_semantics import neighbor_sampler_full
    adj, _, _ = delaunay_tet_graph(points, seed)
    n = adj.shape[0] // 4
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 29, generator=g)
    ea = torch.randn(4 * n, 20, generator=g)
    idx = torch.randperm(n, generator=g)[:batch].numpy()
    n_id, adjs = neighbor_sampler_full(adj.T.astype(np.int64), n, idx, len(convs))
    adjs = [(torch.from_numpy(a), torch.from_numpy(e), s) for a, e, s in adjs]
    G = torch.randn(batch, 2, generator=g)
    net = oracle_static(train=True, dtype=torch.float64, convs=convs, load=shipped, seed=seed + 10)
    if not shipped:
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                    m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                    m.running_mean.copy_(torch.randn(m.num_features, generator=g))
                    m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                    m.num_batches_tracked.fill_(3)
    return net, x, ea, torch.from_numpy(n_id), adjs, G


def static_sd(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def test_static_training_model_without_rounding_is_the_oracle():
    """every rounding site off: static_step's explicit forward / backward == the oracle's autograd step in fp64 -- logits, every parameter gradient
    (BatchNorm's dgamma / dbeta and the biases ahead of a BatchNorm among them), running_mean / running_var after the momentum update and
    num_batches_tracked.  This pins the restatement the GPU test holds the HIP path to."""
    from bf16_training_model import static_step
    from dgnn_amd.config import Config
    convs = (16, 24, 32, 16)
    net, x, ea, n_id, adjs, G = _static_block(500, 24, convs)
    sd = static_sd(net)
    ologits = net(Config(all=Config(x=x.double(), edge_attr=ea.double()), batch_n_id=n_id, batch_adjs=adjs))
    (ologits * G.double()).sum().backward()
    logits, grads, bufs = static_step(sd, convs, x, ea, n_id, adjs, G, sites=())
    assert ologits.shape == logits.shape == (24, 2)
    assert (logits - ologits.detach()).abs().max().item() <= 1e-12 * max(1.0, ologits.abs().max().item())
    ref = {k: p.grad for k, p in net.named_parameters()}
    assert set(ref) == set(grads)
    gmax = max(r.abs().max().item() for r in ref.values())
    for k, r in ref.items():
        # (the biases ahead of a train-mode BatchNorm have an analytically zero gradient: both sides hold fp64 noise there, hence the floor)
        err = (grads[k] - r).abs().max().item()
        assert err <= 1e-11 * r.abs().max().item() + 1e-14 * gmax, (k, err, r.abs().max().item())
    ob = dict(net.named_buffers())
    assert set(ob) == set(bufs)
    for k, b in bufs.items():
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(ob[k]) == 4, (k, b, ob[k])
        else:
            assert (b - ob[k]).abs().max().item() <= 1e-12 * max(1.0, ob[k].abs().max().item()), k
            assert (b - sd[k].double()).abs().max().item() > 1e-3, k          # the step did move the buffer


def static_spread(points, batch, convs, shipped, threads=8, families=()):
    """-> (the model in fp32 arithmetic against itself in fp64, all sites: {param: structured stats}, and for every family in `families` the model
    with that family left out against the full model in fp64: {family: {param: structured stats}}).  Stats as grad_bound_stats."""
    from bf16_training_model import STATIC_SITES, static_step
    torch.set_num_threads(threads)
    net, x, ea, n_id, adjs, G = _static_block(points, batch, convs, shipped=shipped)
    sd = static_sd(net)
    l64, g64, b64 = static_step(sd, convs, x, ea, n_id, adjs, G)
    l32, g32, b32 = static_step(sd, convs, x, ea, n_id, adjs, G, arith=torch.float32)
    spread = dict(logits=_logit_stats(l64, l32), grads=grad_bound_stats(g64, g32), bufs=_buf_stats(b64, b32), cells=int(n_id.numel()))
    off = {}
    for fam in families:
        _, gf, _ = static_step(sd, convs, x, ea, n_id, adjs, G, sites=STATIC_SITES - {fam})
        off[fam] = grad_bound_stats(g64, gf)
    return spread, off


def _logit_stats(ref, got):
    d = (got - ref).abs()
    return dict(equal=(d == 0).double().mean().item(), max=d.max().item(), top=ref.abs().max().item())


def _buf_stats(ref, got):
    return {k: ((got[k].double() - ref[k].double()).abs().max().item() / max(ref[k].double().abs().max().item(), 1e-30)) for k in ref
            if not k.endswith("num_batches_tracked")}


def grad_bound_stats(ref, got):
    """what the GPU test's structured bound looks at, per tensor: rms of the difference relative to the tensor's rms, max relative to its largest
    entry, and the number of entries beyond fp32 class (see test_gpu_scale.py::assert_grads_within_rounding_model)"""
    mmax = max(r.abs().max().item() for r in ref.values())
    out = {}
    for k, r in ref.items():
        d = (got[k].double() - r).abs()
        top = r.abs().max().item()
        rrms = max(r.pow(2).mean().sqrt().item(), 1e-300)
        line = max(d.pow(2).mean(dim=1).sqrt().max().item(), d.pow(2).mean(dim=0).sqrt().max().item()) / rrms if d.dim() == 2 else 0.0
        out[k] = dict(rms=d.pow(2).mean().sqrt().item() / rrms, max=d.max().item() / max(top, 1e-300), line=line,
                      outside=int((d > 1e-3 * top + 1e-6 * mmax).sum().item()), n=d.numel())
    return out


ZERO_GRAD = lambda k: k.endswith("conv.lin_j.bias") or k == "decoder.0.bias"      # biases ahead of a train-mode BatchNorm: analytically zero


@pytest.mark.parametrize("points,batch,convs,shipped", [(30000, 2048, (64, 128, 128, 128), True), (10000, 1024, (128, 256, 512, 1024), False)])
def test_static_rounding_model_spread_sets_the_gpu_bound(points, batch, convs, shipped):
    """static_step in fp32 arithmetic against itself in fp64, all sites on, at the GPU test's sizes: what two CORRECT implementations of the model
    differ by.  Measured (worst tensor): rms 3.3e-2 / 4.2e-2, entry 6.7e-2 / 1.5e-1 of the largest, row or column 0.24 / 0.24 of the rms; the GPU
    bound (STATIC_BF16_*) keeps 1.4x .. 2x of room above that."""
    from bf16_training_model import STATIC_BF16_CAP, STATIC_BF16_LINE, STATIC_BF16_RMS
    spread, _ = static_spread(points, batch, convs, shipped, threads=min(os.cpu_count() or 8, 16))
    g = {k: v for k, v in spread["grads"].items() if not ZERO_GRAD(k)}
    worst = {q: max(v[q] for v in g.values()) for q in ("rms", "max", "line")}
    assert 1e-3 < worst["rms"] <= STATIC_BF16_RMS / 1.4 and worst["max"] <= STATIC_BF16_CAP / 1.4 and worst["line"] <= STATIC_BF16_LINE / 1.4, worst
    assert spread["logits"]["max"] <= 2.0 ** -7 * spread["logits"]["top"] and max(spread["bufs"].values()) <= 1e-5, spread


def test_static_rounding_sites_that_the_gpu_bound_sees():
    """Leaving out one site family moves the worst gradient tensor by more than the GPU bound for every FORWARD family (x, w, a, z, y: measured
    0.10-0.18 rms at the GPU test's sizes), and for the backward families (dy, dz, da, dx, dxacc: 0.4-0.9e-2) by less than the spread of two
    correct implementations -- a whole-step comparison cannot see those; the kernel-level tests hold them (see the GPU test)."""
    from bf16_training_model import STATIC_BF16_RMS
    fams = ("x", "w", "a", "z", "y", "dy", "dz", "da", "dx", "dxacc")
    _, off = static_spread(10000, 1024, (64, 128, 128, 128), True, threads=min(os.cpu_count() or 8, 16), families=fams)
    worst = {f: max(v["rms"] for k, v in off[f].items() if not ZERO_GRAD(k)) for f in fams}
    for f in ("x", "w", "a", "z", "y"):
        assert worst[f] > 1.5 * STATIC_BF16_RMS, worst
    for f in ("dy", "dz", "da", "dx", "dxacc"):
        assert 1e-3 < worst[f] < STATIC_BF16_RMS, worst      # present (a real rounding of the path) but below the bound
