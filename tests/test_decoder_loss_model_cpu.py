"""tests/decoder_loss_model.py held to torch: the fp64 references against the torch modules and op chains they restate, the operand splits
against their definition, and the exactness of the exact input families proved by sequential fp32 evaluation.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

import decoder_loss_model as dm
import gemm_model as gm


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- decoder ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", [o for o in dm.ALL_OPTS if o.ldo == o.n_out], ids=lambda o: "n%d-b0%d-ss%d-b3%d" % o[:4])
def test_ref_decoder_is_the_two_linear_module_in_float64(o):
    """Linear(128, 64) -> BatchNorm(eval) as scale / shift -> ReLU -> Linear(64, n_out) built from torch modules in float64; the magnitude
    bounds the result and is the result on non-negative inputs"""
    d = dm.with_opts(dm.range_decoder(37, "wide", _gen(5)), o)
    l0, l3 = torch.nn.Linear(128, 64, bias=o.b0, dtype=torch.float64), torch.nn.Linear(64, o.n_out, bias=o.b3, dtype=torch.float64)
    with torch.no_grad():
        l0.weight.copy_(d.W0)
        l3.weight.copy_(d.W3)
        if o.b0:
            l0.bias.copy_(d.b0)
        if o.b3:
            l3.bias.copy_(d.b3)
        h = l0(d.y.double())
        if o.ss:
            h = h * d.scale.double() + d.shift.double()
        want = l3(torch.relu(h))
    got, mag = dm.ref_decoder(*d)
    assert (got - want).abs().max() <= 1e-12 * mag.max()
    assert (got.abs() <= mag * (1 + 1e-12)).all()
    pos = dm.DecoderInputs(*(None if t is None else t.abs() for t in d))
    r, m = dm.ref_decoder(*pos)
    assert torch.allclose(m, 2 * r - (0 if pos.b3 is None else pos.b3.double()), rtol=1e-12)     # |W3| m1 = |W3| h there: m = 2 W3 h + b3


def test_ref_decoder_options_are_not_silently_equal():
    d = dm.range_decoder(9, "randn", _gen(1))
    outs = [dm.ref_decoder(*dm.with_opts(d, o))[0] for o in dm.ALL_OPTS if o.n_out == 2 and o.ldo == 2]
    for i in range(len(outs)):
        for j in range(i):
            assert not torch.equal(outs[i], outs[j])


def _is_bf16_value(t):
    return torch.equal(gm.bf16_round(t), t)


def test_splits_readd_and_every_part_is_bf16():
    """split3: three bf16 parts that re-add to all 24 bits; split2: two parts that re-add to 16 bits (error at most 2^-17 |x|, and exact on
    16-bit inputs)"""
    g = _gen(2)
    x = gm.wide((300, 64), g, (-20, 20))
    hi, mid, lo = dm.split3(x)
    assert all(_is_bf16_value(p) for p in (hi, mid, lo))
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    h2, l2 = dm.split2(x)
    assert _is_bf16_value(h2) and _is_bf16_value(l2) and torch.equal(h2, hi)
    assert ((h2.double() + l2.double() - x.double()).abs() <= 2.0 ** -17 * x.double().abs()).all()
    assert (l2 != 0).float().mean() > 0.9
    v = dm.two_part((64, 128), g)
    h2, l2 = dm.split2(v)
    assert torch.equal(h2.double() + l2.double(), v.double()) and (l2 != 0).all() and (h2 != 0).all()
    t = gm.three_part((64, 16), g)
    hi, mid, lo = dm.split3(t)
    assert (hi != 0).all() and (mid != 0).all() and (lo != 0).all()


def test_w0_as_seen():
    W0 = torch.randn(64, 128, generator=_gen(3))
    hi, lo = dm.split2(W0)
    assert torch.equal(dm.w0_as_seen(W0, "rows"), W0.double()) and torch.equal(dm.w0_as_seen(W0, "fused_stride"), W0.double())
    assert torch.equal(dm.w0_as_seen(W0, "bf16_single"), hi.double())
    assert torch.equal(dm.w0_as_seen(W0, "bf16_comp"), hi.double() + lo.double())
    assert not torch.equal(dm.w0_as_seen(W0, "bf16_comp"), hi.double()) and not torch.equal(dm.w0_as_seen(W0, "bf16_comp"), W0.double())


@pytest.mark.parametrize("tile_tag", [False, True])
def test_exact_decoder_inputs_are_exact_in_fp32(tile_tag):
    """the sequential fp32 evaluation equals fp64 bit for bit under every option set, every value is a bf16 value (the bf16 decoder stores y so),
    and the sum of all magnitudes stays below 2^24 halves"""
    M = 97 * 32 + 5 if tile_tag else 131
    d = dm.exact_decoder(M, _gen(7), tile_tag)
    assert _is_bf16_value(d.y) and _is_bf16_value(d.W0)
    for o in dm.ALL_OPTS:
        if o.ldo != o.n_out:
            continue
        a = dm.with_opts(d, o)
        ref, mag = dm.ref_decoder(*a)
        assert mag.max() < 1e6 and mag.max() * 2 < 2.0 ** 24
        assert torch.equal(dm.seq_decoder_fp32(*a).double(), ref), o
        assert torch.equal(ref * 2, (ref * 2).round())
    if tile_tag:
        tiles = d.y[::32, :2]
        assert torch.unique(tiles, dim=0).size(0) == tiles.size(0)


@pytest.mark.parametrize("which", ["y3", "W0_3", "W0_2"])
def test_parts_decoder_is_exact_and_needs_every_part(which):
    """the parts cases: sequential fp32 == fp64 bit for bit, all terms of a logit are multiples of one unit and their magnitudes sum to less
    than 2^24 of it (so every order and every split is exact too); without the mid or the lo part of the multi-part operand most rows change"""
    d = dm.parts_decoder(257, which, _gen(11))
    for n_out in (1, 2):
        a = dm.with_opts(d, dm.Opt(n_out, True, False, True, n_out))
        ref, _ = dm.ref_decoder(*a)
        assert torch.equal(dm.seq_decoder_fp32(*a).double(), ref)
        _, m1 = gm.ref_fwd(a.y, a.W0, bias=a.b0)
        terms = m1 @ a.W3.double().abs().t() + a.b3.double().abs()
        unit = dm.parts_unit(d, which)[:, :n_out]
        assert (terms / unit).max() < 2.0 ** 24
        assert torch.equal(ref / unit, (ref / unit).round())
        for part in (("lo2",) if which == "W0_2" else ("mid", "lo")):
            b = a._replace(y=dm.drop_part(a.y, part)) if which == "y3" else a._replace(W0=dm.drop_part(a.W0, part))
            changed = (dm.ref_decoder(*b)[0] != ref).any(dim=1).float().mean().item()
            assert changed > 0.5, (which, part, changed)
    if which == "W0_2":
        assert torch.equal(dm.w0_as_seen(d.W0, "bf16_comp"), d.W0.double()) and _is_bf16_value(d.y)
    else:
        used = sorted(set((c // 16, (c % 16) // 8) for c in dm.PARTS_COLS))
        assert used == [(S, g) for S in range(8) for g in range(2)]
        assert (d.W3[:, :32] != 0).any(dim=1).all() and (d.W3[:, 32:] != 0).any(dim=1).all()


# ---- loss ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "fitted"])
@pytest.mark.parametrize("norm", dm.NORMS)
def test_ref_kl_is_the_reference_op_chain_in_float64(norm, kind):
    """F.kl_div(F.log_softmax(...)), the three weights, both sums, the quotient and the autograd gradient in float64, at 1e-12 of the magnitudes"""
    logits, gt, vol = dm.range_rows(3001, kind, _gen(norm + 20))
    r = dm.ref_kl(logits, gt, vol, norm, 1.7)
    s, w, loss, g = dm.chain(logits.double(), gt.double(), vol.double(), norm, 1.7)
    scale = (r.mu * r.w).sum()
    assert abs(s - r.sum_cw) <= 1e-12 * scale and abs(w - r.sum_w) <= 1e-12 * r.sum_w
    assert abs(loss - r.loss) <= 1e-12 * scale / r.sum_w
    assert ((g - r.dlogits).abs() <= 1e-12 * r.grad_mag + 1e-300).all()
    assert (r.dlogits.abs() <= r.grad_mag * (1 + 1e-12)).all() and abs(r.sum_cw) <= scale
    if kind == "fitted":
        assert abs(r.loss) < 1e-6 and scale / r.sum_w > 0.1          # the loss cancels; its terms do not
    else:
        tt = gt.sum(1)
        assert (tt - 1).abs().max() > 0.4 and (gt == 0).any() and (gt == 1).any() and (logits[:, 1] - logits[:, 0]).abs().max() > 100


def test_ref_kl_gradient_carries_the_target_sum():
    logits, gt, vol = dm.range_rows(500, "mixed", _gen(4))
    r = dm.ref_kl(logits, gt, vol, 0)
    unit = dm.ref_kl(logits, gt / gt.sum(1, keepdim=True), vol, 0)
    assert (r.dlogits - unit.dlogits).abs().max() > 1e-3 * r.grad_mag.max()


@pytest.mark.parametrize("n", [1, 64, 1025, 5000])
def test_saturated_rows_are_exact_in_fp32(n):
    """expf(-d) = 0 and logf(1) = 0 in fp32: the reference's fp32 chain gives cell terms of exactly 0 or d, the fp64 model the same integers, and
    both agree with the sums read off the rows' definition"""
    logits, gt, vol = dm.saturated_rows(n, _gen(n))
    want = dm.saturated_sums(logits, gt, vol)
    cell = F.kl_div(F.log_softmax(logits, dim=-1), gt, reduction="none").sum(dim=1)
    d = (logits[:, 0] - logits[:, 1]).abs()
    assert ((cell == 0) | (cell == d)).all() and d.min() >= 128 and d.max() <= 512
    assert (cell.double() * vol.double()).sum() == want[0]
    r = dm.ref_kl(logits, gt, vol, 0)
    assert r.sum_cw == want[0] and r.sum_w == want[1] and r.oa == want[2]
    assert want[0] < 2.0 ** 53 and torch.equal(want, want.round())
    if n >= 64:
        assert 0 < want[2] < n and 0 < want[0]


def test_oa_rule_is_the_reference_s_argmax_of_the_fp32_log_softmax():
    """rows with l1 - l0 in {0, 1e-10, 1e-8, 1.2e-7, -1e-10} (and mirrored): the restated rule against F.log_softmax(...).argmax(1) in float32,
    on both sides of t0 > t1 and on t0 == t1; below 3e-8 the reference counts class 0 where the larger logit says 1"""
    L, T = dm.oa_edge_rows()
    want = F.log_softmax(L, dim=-1).argmax(1)
    assert torch.equal(dm.oa_pred(L), want)
    diffs = [d for d in dm.OA_DIFFS for _ in dm.OA_TARGETS]
    for d, p, row in zip(diffs, want.tolist(), L):
        assert (row[1] > row[0]) == (d > 0) and (row[1] == row[0]) == (d == 0)
        assert p == (1 if d > 3e-8 else 0), (d, p)
    assert sum(1 for d, p, row in zip(diffs, want.tolist(), L) if bool(row[1] > row[0]) != bool(p)) == 6      # the rows the logit rule gets wrong
    vol = torch.ones(L.size(0))
    r = dm.ref_kl(L, T, vol, 0)
    assert r.oa == int(((T[:, 0] > T[:, 1]).long() == want).sum())
    assert r.oa != int(((T[:, 0] > T[:, 1]) == (L[:, 1] > L[:, 0])).sum())
    for n in (300, 5000):
        logits, gt, vol = dm.range_rows(n, "mixed", _gen(n))
        assert torch.equal(dm.oa_pred(logits), F.log_softmax(logits, dim=-1).argmax(1))


def test_loss_bounds_measure_the_fp32_chain():
    """the CPU chain's error in the units of the GPU test's bounds.  The weighted sum: far below 2^-23.  The gradient: up to 3e-6 on the mixed
    rows, where l - max is rounded at a difference of about 100 (half an ulp there is 4e-6, and exp carries it over), 3e-7 on the fitted rows; with the log norm 6e-5 on the mixed rows, which is
    the rounding of 1 + vol at vol = 1e-3 (2^-24 of 1, 6e-5 of log(1 + vol)) -- terms the kernels share, which is why B is measured and not fixed"""
    for norm in dm.NORMS:
        for kind in ("mixed", "fitted"):
            logits, gt, vol = dm.range_rows(70000, kind, _gen(9))
            r = dm.ref_kl(logits, gt, vol, norm, 1.7)
            bs, bg, es, eg = dm.loss_bounds(logits, gt, vol, norm, 1.7, r)
            print("norm %d %s: fp32 chain error %.3g of sum mu w, %.3g of the gradient magnitude" % (norm, kind, es, eg))
            assert dm.LOSS_FLOOR <= bs < 1e-6 and dm.LOSS_FLOOR <= bg < (2e-6 if kind == "fitted" else 1e-3 if norm == 1 else 2e-5)


@pytest.mark.parametrize("norm", dm.NORMS)
def test_rows_built_from_functions_rounded_once_are_within_the_floor_each(norm):
    """the arithmetic of loss.hip (add_row) restated: every single row is within 2^-23 of mu_k w_k (down to fp32's underflow) and its weight within 2^-24 of itself --
    which the reference's plain fp32 chain is not (logf(expf + expf), logf(1.f + vol)) --, and saturated rows stay exactly 0 or d"""
    for kind in ("mixed", "fitted"):
        logits, gt, vol = dm.range_rows(20000, kind, _gen(31 + norm))
        r = dm.ref_kl(logits, gt, vol, norm)
        cw, w = dm.kernel_rows(logits, gt, vol, norm)
        exact = r.cell * r.w
        tiny = dm.TINY * gt.double().abs().sum(dim=1) * r.w              # a log-sum below 2^-126 is a subnormal float or 0
        assert ((cw - exact).abs() <= dm.LOSS_FLOOR * r.mu * r.w + tiny).all()
        assert ((w - r.w).abs() <= 2.0 ** -24 * r.w).all()
        cell32 = F.kl_div(F.log_softmax(logits, dim=-1), gt, reduction="none").sum(dim=1)
        w32 = torch.log(1 + vol) if norm == 1 else (torch.sqrt(vol) if norm == 2 else vol)
        if kind == "mixed":
            assert ((cell32.double() * w32.double() - exact).abs() > dm.LOSS_FLOOR * r.mu * r.w).any()
    logits, gt, vol = dm.saturated_rows(5000, _gen(5))
    cw, w = dm.kernel_rows(logits, gt, vol, 0)
    d = (logits[:, 0] - logits[:, 1]).abs().double()
    assert ((cw == 0) | (cw == d * vol.double())).all() and cw.sum() == dm.saturated_sums(logits, gt, vol)[0]


def test_with_oa_rows_places_them():
    logits, gt, vol = dm.saturated_rows(2049, _gen(1))
    L, T = dm.oa_edge_rows()
    a, b = dm.with_oa_rows(logits, gt, 1024 - 10)
    assert torch.equal(a[1014:1014 + 21], L) and torch.equal(b[1014:1014 + 21], T) and torch.equal(a[:1014], logits[:1014]) and torch.equal(a[1035:], logits[1035:])
