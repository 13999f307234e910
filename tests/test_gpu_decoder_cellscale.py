"""The decoder stages of the last conv layer's launch (k_sage_fused_ws<128, 2, DEC>, dgnn_amd/csrc/fused_ws.hip): one power-of-two scale per cell
for the parked tile (stages A1 / A2), K = 32 products in stage B, the four-stage drain.  Against the CPU oracle with the tolerance of
test_gpu_parity.py::test_last_layer_and_decoder_in_one_launch, and -- for hand-made rows that stress the scale -- against an fp64 evaluation of
the same decoder with a bound derived from the arithmetic."""
import numpy as np
import pytest
import torch

from dgnn_amd.config import Config
from helpers import kf96_state_dict, oracle_static

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL_LOGIT = 1e-4
WS_TILE, NUM_CU = 32, 256


def hip_static(sd=None):
    from dgnn_amd.config import reconbench_pretrained
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import SurfaceNet
    net = SurfaceNet(reconbench_pretrained(device=DEV))
    net.load_state_dict(kf96_state_dict() if sd is None else sd)
    return net.to(DEV).eval()


def one_launch_or_skip(net):
    from dgnn_amd import ops
    if ops.GEMM_MODE != ops.GEMM_F16X2 or not ops.FUSE_DECODER:
        pytest.skip("the one-launch form exists for the default arithmetic only (DGNN_GEMM_MODE / DGNN_FUSE_DECODER select the two-launch form)")
    assert net.fuses_decoder(3)


def tiles_per_workgroup(n_dst):
    """How dgnn_sage_layer_fused_ws_try / k_sage_fused_ws hand the 32-cell tiles of a launch to its workgroups (grid = min(tiles, 256); workgroup
    b serves XCD b % 8, which walks one contiguous eighth of the tiles)."""
    ntiles = -(-n_dst // WS_TILE)
    grid = max(1, min(ntiles, NUM_CU))
    per = (ntiles + 7) // 8
    out = []
    for b in range(grid):
        xcd, slot = b & 7, b >> 3
        wg_per_xcd = (grid + 7 - xcd) >> 3
        t_lo = xcd * per
        t_hi = min(ntiles, t_lo + per)
        out.append((t_hi - t_lo - slot + wg_per_xcd - 1) // wg_per_xcd if t_lo + slot < t_hi else 0)
    assert sum(out) == ntiles
    return out


def scene(points, seed):
    from dgnn_amd.synthetic import delaunay_tet_graph
    adj, _, _ = delaunay_tet_graph(points, seed=seed)
    n = adj.shape[0] // 4
    g = torch.Generator().manual_seed(seed)
    x, ea = torch.randn(n, 29, generator=g), torch.randn(4 * n, 20, generator=g)
    return n, x, ea, torch.from_numpy(adj.T.astype(np.int64))


@pytest.fixture(scope="module")
def small():
    """one scene of some ten thousand cells, its oracle logits and the rows that enter the last conv layer"""
    from dgnn_amd.graph import GraphPlan
    n, x, ea, ei = scene(1500, 5)
    with torch.no_grad():
        ref = oracle_static().inference_layer(Config(x=x, edge_attr=ea, edge_index=ei))
    net = hip_static()
    data = Config(x=x.to(DEV), edge_attr=ea.to(DEV), edge_index=ei.to(DEV))
    plan = GraphPlan(data.edge_index, n, n)
    h = data.x[:, 1:]
    for i in range(3):
        h = net._eval_layers(h, n, data.edge_attr, [plan] * 4, True, only=i)
    return Config(n=n, ref=ref, net=net, data=data, plan=plan, h=h)


def test_whole_graph_below_one_tile():
    n, x, ea, ei = scene(9, 3)
    assert 0 < n < WS_TILE and tiles_per_workgroup(n) == [1]
    net = hip_static()
    one_launch_or_skip(net)
    with torch.no_grad():
        ref = oracle_static().inference_layer(Config(x=x, edge_attr=ea, edge_index=ei))
    data = Config(x=x.to(DEV), edge_attr=ea.to(DEV), edge_index=ei.to(DEV))
    one = net.inference_layer(data)
    assert (one.cpu() - ref).abs().max().item() <= TOL_LOGIT * max(1.0, ref.abs().max().item())
    assert torch.equal(one, net.inference_layer(data))


# launches of 20, 33 and 270 cells and of the whole scene (no multiple of 32): workgroups with one tile; two workgroups with one tile each; nine tiles
# on nine workgroups, which the per-XCD split hands out as 0, 1 and 2 tiles; several tiles per workgroup with a partial last one
@pytest.mark.parametrize("cells,counts", [(20, {1}), (33, {1}), (270, {0, 1, 2}), (None, None)])
def test_drain_with_zero_one_two_tiles_per_workgroup(small, cells, counts):
    s = small
    one_launch_or_skip(s.net)
    k = s.n if cells is None else cells
    assert k <= s.n
    got = set(tiles_per_workgroup(k))
    if counts is None:
        assert s.n % WS_TILE != 0 and max(got) >= 2
    else:
        assert got == counts
    args = (s.h, s.n, s.data.edge_attr, [s.plan] * 4, True)
    whole = s.net._eval_layers(*args, only=3, decode=True)
    out = torch.full((s.n, 2), float("nan"), device=DEV)
    s.net._eval_layers(*args, only=3, out=out, rows=(0, k), decode=True)
    torch.cuda.synchronize()
    tol = TOL_LOGIT * max(1.0, s.ref.abs().max().item())
    err = (out[:k].cpu() - s.ref[:k]).abs().max().item()
    print("cells %d: tiles per workgroup %s, max |dlogit| %.3e (tol %.3e)" % (k, sorted(got), err, tol))
    assert err <= tol
    assert torch.equal(out[:k], whole[:k]) and bool(torch.isnan(out[k:]).all())


def test_many_tiles_per_workgroup_both_buffers_reused():
    """about 20 000 points: every workgroup walks several tiles, so both buffers of the parked tile, of the counters and of the partial logits and
    all four of the per-cell exponent words are re-used"""
    n, x, ea, ei = scene(20000, 7)
    per_wg = tiles_per_workgroup(n)
    assert len(per_wg) == NUM_CU and max(per_wg) >= 5 and min(per_wg) >= 5
    net = hip_static()
    one_launch_or_skip(net)
    with torch.no_grad():
        ref = oracle_static().inference_layer(Config(x=x, edge_attr=ea, edge_index=ei))
    data = Config(x=x.to(DEV), edge_attr=ea.to(DEV), edge_index=ei.to(DEV))
    one = net.inference_layer(data)
    tol = TOL_LOGIT * max(1.0, ref.abs().max().item())
    err = (one.cpu() - ref).abs().max().item()
    print("n %d: tiles per workgroup %d..%d, max |dlogit| %.3e (tol %.3e)" % (n, min(per_wg), max(per_wg), err, tol))
    assert err <= tol
    assert torch.equal(one, net.inference_layer(data))


def stress_rows(n, seed):
    """Rows that come out of the last conv layer unchanged but for the BatchNorm factor (see stress_net): per cell one of eight patterns, so that every
    32-cell tile and both of its row blocks hold all of them"""
    g = torch.Generator().manual_seed(seed)
    h = 1.0 + 0.5 * torch.randn(n, 128, generator=g).abs()
    cell = torch.arange(n)
    pat = cell % 8
    sl = ((cell // 8) % 8)[:, None] == (torch.arange(128) // 16)[None, :]       # the cell's marked 16-channel slice
    small_ = torch.full((n, 128), 2.0 ** -12)
    one_ = torch.ones(n, 128)
    f = one_.clone()
    f = torch.where((pat == 1)[:, None], torch.where(sl, one_, small_), f)      # one slice large, the rest 2^-12 of it
    f = torch.where((pat == 2)[:, None], torch.where(sl, small_, one_), f)      # the reverse
    f = torch.where((pat == 3)[:, None], -one_, f)                              # all zero behind the ReLU
    f = torch.where((pat == 4)[:, None], 1e-20 * one_, f)
    f = torch.where((pat == 5)[:, None], 1e+20 * one_, f)
    f = torch.where((pat == 6)[:, None], 1e+20 * torch.where(sl, one_, small_), f)
    f = torch.where((pat == 7)[:, None], torch.where(torch.rand(n, 128, generator=g) < 0.5, -one_, one_), f)      # half the channels zero
    return (h * f).contiguous(), pat


def stress_net():
    """the shipped decoder behind a last conv layer that hands its own row through: filter and neighbour weights zero, own weights the identity, BatchNorm
    with mean 0 / variance 1 -- y = relu(h / sqrt(1 + eps))"""
    sd = {k: v.clone() for k, v in kf96_state_dict().items()}
    p = "convs.3."
    for k in ("conv.lin_j.weight", "conv.lin_j.bias", "conv.lin_e.weight", "conv.lin_e.bias", "norm.module.bias", "norm.module.running_mean"):
        sd[p + k].zero_()
    sd[p + "conv.lin_i.weight"] = torch.eye(128)
    sd[p + "norm.module.weight"].fill_(1.0)
    sd[p + "norm.module.running_var"].fill_(1.0)
    return hip_static(sd)


def test_scale_stress_against_fp64_decoder():
    """Cells whose 16-channel slices differ by 2^12 (one large, the rest small, and the reverse), all-zero cells, cells at 1e-20 and at 1e+20, driven
    through the last layer's launch directly.  Reference: the decoder in fp64 on the rows y the plain launch of the same layer writes.

    Bound, per cell and logit k, from the arithmetic of stages A2 / B (fused_common.h, the fp16 two-part form):
      * y and W0 each enter with 22 significant bits relative to the largest magnitude of their scaling group (the cell's 128 channels; the 16 rows of a
        hidden block -- no row of the shipped W0 lies 2^15 below its block's maximum, asserted below), and the lo x lo product is dropped: three terms of
        2^-22 ymax |W0[u, c]| per product, summed over c;
      * twelve fp32 accumulations per hidden unit, each rounding a partial sum of at most ymax sum_c |W0[u, c]|: 12 x 2^-24 = 3 x 2^-22 of it;
        together 6 x 2^-22 x ymax x rowsum_u(|W0|) on the hidden pre-activation u, carried to the logit by |A1[u]| |W3[k, u]| (ReLU does not expand it);
      * the fp32 tail (BatchNorm folded in fp32, fma + max, 4 fma per lane, 2 + 4 additions, the bias): at most 16 roundings of 2^-24 on values bounded by
        S_k = sum_u |W3[k, u]| (|A1[u] pre_u| + |B1[u]|) + |b3[k]|.
    Measured worst ratio error / bound on MI355X: 0.024 over all cells (0.024 among the one-slice-large, the all-zero and the 1e-20 cells, where the fp32
    tail against the fp64 reference is most of the error; 0.015 for the reverse pattern; 0.003-0.004 for the cells at 1e+20)."""
    from dgnn_amd.graph import GraphPlan
    n, _, ea, ei = scene(400, 5)
    assert n >= 1024
    net = stress_net()
    one_launch_or_skip(net)
    h, pat = stress_rows(n, 11)
    ei_d, ea_d, h_d = ei.to(DEV), ea.to(DEV), h.to(DEV)
    plan = GraphPlan(ei_d, n, n)
    args = (h_d, n, ea_d, [plan] * 4, True)
    y = net._eval_layers(*args, only=3, decode=False)
    lg = net._eval_layers(*args, only=3, decode=True)
    torch.cuda.synchronize()
    y64 = y.double().cpu()
    # the layer handed the patterns through
    assert torch.equal(y64[pat == 3], torch.zeros_like(y64[pat == 3]))
    ymax = y64.abs().max(dim=1).values
    assert ((y64 - h.double().clamp_min(0)).abs().max(dim=1).values <= 2e-5 * ymax).all()
    assert 1e-21 < ymax[pat == 4].max().item() < 1e-19 and ymax[pat == 5].min().item() > 1e19
    for p_ in (1, 6):
        part = y64[pat == p_]
        srt = part.sort(dim=1).values
        assert (srt[:, 111] * 2.0 ** 9 < srt[:, 112]).all()      # 112 small channels, 16 large ones

    dec = oracle_static(dtype=torch.float64).decoder
    W0, b0, bn, W3, b3 = dec[0].weight, dec[0].bias, dec[1].module, dec[3].weight, dec[3].bias
    with torch.no_grad():
        ref = dec(y64)
        A1 = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        B1 = (b0 - bn.running_mean) * A1 + bn.bias
        blockmax = W0.abs().reshape(4, 16 * 128).max(dim=1).values
        assert (W0.abs().reshape(4, 16, 128).max(dim=2).values > blockmax[:, None] * 2.0 ** -15).all()
        rowsum = W0.abs().sum(dim=1)                                               # [64]
        pre = y64 @ W0.t()
        hid = 6 * 2.0 ** -22 * ymax[:, None] * rowsum[None, :]                     # [n, 64]
        S = (pre * A1).abs() + B1.abs()
        bound = (hid * A1.abs()) @ W3.abs().t() + 16 * 2.0 ** -24 * (S @ W3.abs().t() + b3.abs())
    err = (lg.double().cpu() - ref).abs()
    ratio = err / bound
    for p_ in range(8):
        print("pattern %d: worst error / bound %.3f, worst |error| %.3e" % (p_, ratio[pat == p_].max().item(), err[pat == p_].max().item()))
    assert bool(torch.isfinite(lg).all())
    assert (ratio <= 1.0).all()

    # the same bits run to run and in three destination sub-ranges
    assert torch.equal(lg, net._eval_layers(*args, only=3, decode=True))
    cut = [0, n // 3, n // 3 + 1, n]
    out = torch.full((n, 2), float("nan"), device=DEV)
    for b, e in zip(cut[:-1], cut[1:]):
        net._eval_layers(*args, only=3, out=out, rows=(b, e), decode=True)
    assert torch.equal(out, lg)
