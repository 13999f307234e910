"""The wave-specialised fused launches (csrc/fused_ws.hip) after the consumers' ring reads went to four bases + immediate offsets, the dense-stride
instantiations (ldx == c_in) and the producers' 32-bit loop bookkeeping / lane-layout index loads: every fused launch -- 64 -> 128 plain, 128 -> 128
plain, 128 -> 128 + decoder on fp32 rows, the two plain shapes on the unsigned 16-bit rows -- against the UNFUSED aggregate + GEMM pair
(`SurfaceNet._eval_layers_one`, the reference path of the row-level tests) with the shipped kf96 weights, at the tolerance the row-level test states
(tests/test_gpu_parity.py::test_fused_layers_row_level_on_larger_graph: 2e-5 of the layer's largest value per element; logits: TOL_LOGIT scaled as in
test_per_layer_activations_vs_oracle), and each launch repeated bit for bit.  Shapes = the smallest at which this code can go wrong:
  n_dst 1, 3, 31, 32, 33      a short last producer group, the tile edge;
  32 * 256 * 3 + 7            every workgroup walks 3-4 tiles: with two ring slots each is reused (a wrong slot stride or base shows), the decoder's
                              parity buffers too; 32 * 256 * 5 + 7 for the 64-wide 16-bit rows, whose ring has four slots;
  a ragged graph              cells of in-degree 0 .. 9 between regular groups: the per-lane producer path, and first edges off any 16-byte boundary
                              under the 16-byte index load;
  a strided input             ldx != c_in (a column slice of a wider tensor): the run-time-stride instantiation, same bits as the dense one."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, TOL_LOGIT, hip_static
from test_gpu_ws import _graph

pytestmark = pytest.mark.gpu

N_REUSE = 32 * 256 * 3 + 7
SHAPES = [(1, False), (3, False), (31, False), (32, False), (33, False), (N_REUSE, False), (32 * 9 + 5, True)]
LAUNCHES = {"64to128": 1, "128to128": 2, "128to128_decoder": 3}      # launch -> conv layer of the shipped chain


@functools.lru_cache(maxsize=None)
def _net():
    return hip_static()


@functools.lru_cache(maxsize=None)
def _case(n, ragged, c_in):
    """(plan, x [n, c_in] >= 0 as behind a ReLU, edge rows) on the device, built once per shape"""
    from dgnn_amd.graph import GraphPlan
    ei = torch.from_numpy(_graph(n, 17 * c_in + n, ragged)).to(DEV)
    g = torch.Generator().manual_seed(3 * n + c_in)
    x = torch.relu(torch.randn(n, c_in, generator=g))
    x[::37] *= 50.0                                # rows far apart in magnitude: the per-row power-of-two scales
    ea = torch.randn(ei.size(1), 20, generator=g)
    return GraphPlan(ei, n, n), x.to(DEV), ea.to(DEV), ei


def _params(net, i):
    conv = net.convs[i][0]
    scale, shift = net._layer_fold(i)
    return conv.lin_e.weight, conv.lin_e.bias, conv.lin_j.weight, conv.lin_j.bias, conv.lin_i.weight, scale, shift


def _need_ws(ops, dec=False, rows16=False):
    if not ops.lib().dgnn_wave_specialised_enabled() or (not rows16 and ops.GEMM_MODE != ops.GEMM_F16X2) or (dec and not ops.FUSE_DECODER) \
            or (rows16 and ops.BF16_MODE != ops.BF16_COMPENSATED):
        pytest.skip("the wave-specialised kernel runs the default arithmetic (DGNN_GEMM_MODE / DGNN_WS / DGNN_FUSE_DECODER / DGNN_BF16_MODE select others)")


@pytest.mark.parametrize("n,ragged", SHAPES)
@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_fused_launch_vs_unfused_pair_fp32_rows(launch, n, ragged):
    from dgnn_amd import ops
    i = LAUNCHES[launch]
    dec = launch.endswith("decoder")
    _need_ws(ops, dec=dec)
    net = _net()
    c_in = net.convs[i][0].lin_j.in_features
    plan, x, ea, _ = _case(n, ragged, c_in)
    with torch.no_grad():
        ref = net._eval_layers_one(i, x, ea, plan)
        if dec:
            ref = net._eval_decoder(ref)
        P = [t.detach() for t in _params(net, i)]
        D = [t.detach() if t is not None else None for t in net._decoder_args()] if dec else None

        def run(xs):
            if dec:
                return ops.sage_layer_fused_decoder_fwd(plan.rowptr, plan.src, n, xs, ea, *P, True, *D, eid=plan.eid)
            return ops.sage_layer_fused_fwd(plan.rowptr, plan.src, n, xs, ea, *P, True, eid=plan.eid)

        out = run(x)                                # dense rows: ldx == c_in
        again = run(x)
        wide = torch.zeros(n, c_in + 12, device=DEV)
        xs = wide[:, :c_in]                         # ldx = c_in + 12: rows 16-byte aligned, the stride a run-time value
        xs.copy_(x)
        strided = run(xs)
    err = float((out - ref).abs().max())
    tol = TOL_LOGIT * max(1.0, float(ref.abs().max()) / 8) if dec else 2e-5 * float(ref.abs().max())
    print("%s n=%d ragged=%s: max err %.3e, tolerance %.3e" % (launch, n, ragged, err, tol))
    assert out.shape == ref.shape and err <= tol, (err, tol)
    assert torch.equal(out, again)
    assert torch.equal(out, strided)


@pytest.mark.parametrize("launch,n,ragged", [(l, n, r) for l in ("64to128", "128to128") for n, r in SHAPES] + [("64to128", 32 * 256 * 5 + 7, False)])
def test_fused_launch_vs_unfused_pair_16_bit_rows(launch, n, ragged):
    from dgnn_amd import ops
    from test_gpu_bf16 import EPS, _ub_decode, _ub_round
    _need_ws(ops, rows16=True)
    i = LAUNCHES[launch]
    net = _net()
    c_in = net.convs[i][0].lin_j.in_features
    plan, x, ea, _ = _case(n, ragged, c_in)
    xr = _ub_round(x.cpu())
    xin = ((xr.view(torch.int32) >> 15).to(torch.int16)).to(DEV)       # the rows as a previous layer stores them
    with torch.no_grad():
        ref = net._eval_layers_one(i, xr.to(DEV), ea, plan).double().cpu()
        P = [t.detach() for t in _params(net, i)]
        run = lambda xs: ops.sage_layer_fused_fwd_bf16(plan.rowptr, plan.src, n, xs, c_in, ea, *P, True, eid=plan.eid, rows_out_unsigned=True)
        out = run(xin)
        again = run(xin)
        wide = torch.zeros(n, c_in + 16, dtype=torch.int16, device=DEV)
        xs = wide[:, :c_in]
        xs.copy_(xin)
        strided = run(xs)
    assert out.dtype == ops.UROWS and out.shape == (n, 128)
    err = (_ub_decode(out) - ref).abs()
    # the stored value is off by at most half of the format's spacing (EPS = 2^-8 of the value), on top of the row-level tolerance
    bound = 0.5 * EPS * ref.abs() + 2e-5 * float(ref.abs().max()) + 1e-30
    print("%s n=%d ragged=%s: max err / bound %.3f" % (launch, n, ragged, float((err / bound).max())))
    assert bool((err <= bound).all()), (float((err / bound).max()), int((err > bound).sum()))
    assert torch.equal(out, again)
    assert torch.equal(out, strided)
