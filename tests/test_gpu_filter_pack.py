"""The filter product of the fused fp16 two-part kernels on the GPU: the two-product form of the wave-specialised layers (csrc/filter_pack.h, fused_ws.hip:
c_in 64, 128, 128 with the decoder) and, under the same probes, the three products of the first layer's two-phase kernel (fused_mfma.hip: c_in 29).

phi = [A | 1] . [We^T ; be] runs as two v_mfma_f32_16x16x32_f16 whose 64 K-slots hold the 62 real terms (hi.hi, hi.lo, lo.hi).  A term in the wrong slot, on
the wrong k or dropped is about 2^-12 of its product -- far outside the 2^-19 (layers) / 2^-18 (logits) of the terms' magnitude that tests/test_gpu_ws.py
states for these kernels -- provided the inputs make every term count, so the edge rows here are probes: edge e carries ONE non-zero attribute, at
position e mod 20, of value 1 + 2^-12 (its lo part is non-zero, and with the constant slot it is the whole row: each k meets the bias alone); some rows are
dense with a 2^20 spread in magnitude; some are all zero.  We and be are q (1 + 2^-12) with short q: every lo part of the weights is non-zero too.
70 cells of in-degree 4: two full tiles, a partial third, a short last producer group.  fp64 reference; plan-order against eid-gathered attributes and a range
split against the whole run bit for bit.
What the probes catch: a build whose map lacked ONE word (h0,1 . bl0,1) missed the bounds 66-fold (c_in 64), 28-fold (128) and 38-fold (decoder); the shipped
one stays under a tenth of them."""
import numpy as np
import pytest
import torch

from test_gpu_parity import DEV
from test_gpu_ws import BOUND_SCALE, _graph, _reference

pytestmark = pytest.mark.gpu

N = 70
EPS12 = 1.0 + 2.0 ** -12


def _probe_inputs(c_in, c_out, E, seed, one_sign=False):
    """one_sign: every input non-negative and the own-row half, the biases and the shifts small -- a term that went missing is then missing with ONE sign in
    every channel and reaches a logit undiluted through the two dense products behind the filter (with signs at random a lost 2^-12 of one k shrinks by the
    square roots of 128 and 64 on its way and hides under 2^-18 of the logit's terms)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(N, c_in, generator=g)) + 0.25
    e = torch.arange(E)
    ea = torch.zeros(E, 20)
    ea[e, e % 20] = EPS12                                          # one attribute per edge, lo part non-zero
    dense = (e % 7) == 3
    spread = torch.exp2(torch.randint(0, 21, (E, 20), generator=g).float())     # 2^0 .. 2^20 inside one row
    ea[dense] = (torch.randn(E, 20, generator=g) * spread * 2.0 ** -10)[dense]
    ea[(e % 31) == 5] = 0.0                                        # all-zero rows (the scale of the row is then the constant slot's)
    q = lambda *shape: (torch.randint(1, 64, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)) / 32.0
    We, be = q(c_in, 20) * EPS12, q(c_in) * EPS12
    Wj, Wi, bj = torch.randn(c_out, c_in, generator=g) * 0.1, torch.randn(c_out, c_in, generator=g) * 0.1, torch.randn(c_out, generator=g)
    scale, shift = torch.rand(c_out, generator=g) + 0.5, torch.randn(c_out, generator=g)
    if one_sign:
        ea, We, be, Wj = ea.abs(), We.abs(), be.abs(), Wj.abs()
        Wi, bj, shift = Wi * 0.01, bj * 0.01, shift * 0.01
    return x, ea, We, be, Wj, bj, Wi, scale, shift


def _default_arithmetic(ops, decoder=False):
    if ops.GEMM_MODE != ops.GEMM_F16X2 or (decoder and not ops.FUSE_DECODER):
        pytest.skip("the two-product filter form belongs to the default arithmetic (DGNN_GEMM_MODE / DGNN_FUSE_DECODER select other kernels)")


CUT = [0, 20, 28, N]      # (multiples of 4: a cell's group of four is the whole launch's)


@pytest.mark.parametrize("c_in,c_out", [(29, 64), (64, 128), (128, 128)])
def test_filter_products_of_a_layer_vs_fp64(c_in, c_out):
    from dgnn_amd import ops
    _default_arithmetic(ops)
    ei = torch.from_numpy(_graph(N, 900 + c_in, False))
    x, ea, We, be, Wj, bj, Wi, scale, shift = _probe_inputs(c_in, c_out, ei.size(1), c_in)
    ref, mag = _reference(x, ea, ei, N, We, be, Wj, bj, Wi, scale, shift)
    rowptr, src, eid = ops.plan_build(ei.to(DEV), N, 1, n_other=N)
    xs, ead = x.to(DEV), ea.to(DEV)                                # dense rows: stride c_in (29: the first layer's rows as the caller holds them)
    par = [t.to(DEV) for t in (We, be, Wj, bj, Wi, scale, shift)]
    out = ops.sage_layer_fused_fwd(rowptr, src, N, xs, ead, *par, True, eid=eid)
    err = (out.cpu().double() - ref).abs()
    bound = BOUND_SCALE * 2.0 ** -19 * mag + 1e-30
    print("c_in %d: max err / bound = %.3f" % (c_in, float((err / bound).max())))
    assert bool((err <= bound).all()), (float((err / bound).max()), int((err > bound).sum()))
    # edge rows already in plan order (eid = None): the same bits
    assert torch.equal(out, ops.sage_layer_fused_fwd(rowptr, src, N, xs, ead[eid.long()], *par, True))
    # a range split: every cell's row bit for bit
    parts = torch.full_like(out, float("nan"))
    for b, e in zip(CUT[:-1], CUT[1:]):
        ops.sage_layer_fused_fwd(rowptr[b:e + 1], src, e - b, xs, ead, *par, True, eid=eid, x_dst=xs[b:e], out=parts[b:e])
    assert torch.equal(parts, out)


def test_filter_products_of_the_last_layer_with_the_decoder_vs_fp64():
    from dgnn_amd import ops
    _default_arithmetic(ops, decoder=True)
    ei = torch.from_numpy(_graph(N, 7700, False))
    x, ea, We, be, Wj, bj, Wi, scale, shift = _probe_inputs(128, 128, ei.size(1), 77, one_sign=True)
    g = torch.Generator().manual_seed(78)
    W0, b0 = torch.randn(64, 128, generator=g).abs() * 0.15, torch.randn(64, generator=g) * 0.01
    s1, h1 = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.01
    W3, b3 = torch.randn(2, 64, generator=g).abs() * 0.3, torch.randn(2, generator=g) * 0.01
    d = lambda t: t.double()
    ref, mag = _reference(x, ea, ei, N, We, be, Wj, bj, Wi, scale, shift)
    lref = torch.relu((ref @ d(W0).t() + d(b0)) * d(s1) + d(h1)) @ d(W3).t() + d(b3)
    lmag = (((mag @ d(W0).abs().t() + d(b0).abs()) * d(s1).abs() + d(h1).abs()) @ d(W3).abs().t()) + d(b3).abs()
    rowptr, src, eid = ops.plan_build(ei.to(DEV), N, 1, n_other=N)
    xs, ead = x.to(DEV), ea.to(DEV)
    par = [t.to(DEV) for t in (We, be, Wj, bj, Wi, scale, shift)]
    dec = [t.to(DEV) for t in (W0, b0, s1, h1, W3, b3)]
    lg = ops.sage_layer_fused_decoder_fwd(rowptr, src, N, xs, ead, *par, True, *dec, eid=eid)
    err = (lg.cpu().double() - lref).abs()
    bound = BOUND_SCALE * 2.0 ** -18 * lmag + 1e-30
    print("decoder: max err / bound = %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all()), (float((err / bound).max()), int((err > bound).sum()))
    assert torch.equal(lg, ops.sage_layer_fused_decoder_fwd(rowptr, src, N, xs, ead[eid.long()], *par, True, *dec))
    parts = torch.full_like(lg, float("nan"))
    for b, e in zip(CUT[:-1], CUT[1:]):
        ops.sage_layer_fused_decoder_fwd(rowptr[b:e + 1], src, e - b, xs, ead, *par, True, *dec, eid=eid, x_dst=xs[b:e], out=parts[b:e])
    assert torch.equal(parts, lg)
