"""The two-phase fused SAGE inference layers on their own -- k_sage_fused (csrc/fused.hip: f32 with and without the matrix-core filter product, bf16x3) and
k_sage_fused_mfma (csrc/fused_mfma.hip: bf16x3f, f16x2d, f16x2, the decoder-carrying DEC form, the prepared-parameter entry points) -- every output element
against fp64 on the same inputs with a bound proportional to the magnitude of the terms that were added up (tests/fused_layer_model.py; what
tests/test_gpu_ws.py does for the wave-specialised kernel), at the cell counts, in-degrees and row layouts where these kernels take another path.

Shapes and the kernel each reaches in a default process (dgnn_sage_layer_fused_fwd / dgnn_sage_layer_fused_mfma_try / fused_decoder_impl; restated as
fused_layer_model.family_of):

  c_in -> c_out                       modes                       kernel
  28->64, 20->128, 32->128, 64->64    all five                    fused.hip for f32 / bf16x3, fused_mfma.hip for bf16x3f / f16x2d / f16x2
  48->128, 96->128                    all five                    the same; in f16x2 the two-phase (2, 2) form at cin_pad 64 / 128, which the wave-specialised
                                                                  kernel does not take
  29->64 (odd), 100->128 (no          bf16x3f, f16x2d, f16x2      fused_mfma declines (c_in is no multiple of cin_pad / 16), so fused.hip MODE 1; f32 / bf16x3 run
  multiple of 8)                                                  here too (fused.hip MODE 0 with the masked matrix-core filter product, MODE 1)
  64->128, 128->128                   f32, bf16x3, bf16x3f,       two-phase; f16x2 goes to the wave-specialised kernel unless DGNN_WS=0 (this file runs it there as
                                      f16x2d                      well, at the same 2^-19; tests/test_gpu_ws.py owns that kernel's edges)
  decoder launch, c_in 72, 96         f16x2                       fused_mfma.hip DEC (cin_pad 128); c_in = 128 reaches it under DGNN_WS=0 only

The 28- and 29-column rows are passed as a scene passes them: a [:, 1:] view of a wider tensor (row stride no multiple of 4 floats, 4-byte aligned); the
others once contiguous and once with a stride of c_in + 12.  Columns outside a row hold NaN, and so do the rows behind the result.

Bounds (kappa x magnitude, + 1e-30): 2^-19 for f16x2 / f16x2d (22 significand bits per operand, fp32 accumulation: the bound of tests/test_gpu_ws.py), 2^-20
for f32 / bf16x3 / bf16x3f (a plain fp32 evaluation measures at most 0.28 of it, tests/test_fused_layer_model_cpu.py; the kernels make the same number of fp32
roundings in a blocked order, bf16x3 drops terms <= 2^-25 relative), 2^-18 on the logits' magnitude for the decoder launch.  DGNN_TEST_BOUND_SCALE scales them.

Same bits: edge rows through eid / in plan order, padded / contiguous rows, repeats, prepared parameters, destination sub-ranges.  On a 4-regular graph a
cell's row does not depend on where the tile grid cuts the graph (fused_mfma.hip: a short last group stays on the matrix cores; fused.hip: its per-lane path
runs the same chains), so every cut gives the whole launch's bits; on a ragged graph a cut regroups the cells behind it, so only the whole groups before the
cut keep their bits and the rest stays within the bound (the rule tests/test_gpu_wide.py states for the wide aggregate).

The largest err / bound of every (shape, mode) is printed (-s) when the module is done.  Measured on an MI355X over all shapes and sizes: fused.hip f32 0.33,
bf16x3 0.25, MODE 1 under bf16x3f / f16x2d / f16x2 (29, 100 wide) 0.13 / 0.06 / 0.06; fused_mfma.hip bf16x3f 0.28, f16x2d 0.11, f16x2 0.11; the wave-specialised
kernel 0.08; the decoder launch 3.8e-4 (its bound is the worst case of 128 x 64 sums whose errors average out: test_fused_layer_model_cpu.py says what it holds).
"""
import os

import numpy as np
import pytest
import torch

import fused_layer_model as fm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
BOUND_SCALE = float(os.environ.get("DGNN_TEST_BOUND_SCALE", "1"))      # (< 1: how much margin the stated bounds have on this box)
SHAPES = [(28, 64), (20, 128), (32, 128), (64, 64), (48, 128), (96, 128), (29, 64), (100, 128), (64, 128), (128, 128)]
RAGGED_AT_DEPTH = {(28, 64), (20, 128), (64, 64), (48, 128), (96, 128)}      # one shape per instantiation (cin_pad, c_out, family); the others run a 4-regular graph there
WORST = {}


def _ws_enabled():
    from dgnn_amd import ops
    return bool(ops.lib().dgnn_wave_specialised_enabled())


def _layouts(c_in):
    return ("view",) if c_in in (28, 29) else ("padded", "contiguous")


def _rows(x, layout):
    """x on the device in one of the three row layouts; what lies between the rows is NaN"""
    n, c = x.shape
    if layout == "contiguous":
        return x.to(DEV)
    buf = torch.full((n, c + 1) if layout == "view" else (n, c + 12), NAN, device=DEV)
    v = buf[:, 1:] if layout == "view" else buf[:, :c]
    v.copy_(x)
    return v


def _geometry(c_in, c_out, mode, layout, ws_enabled):
    """(family, TILE, cells per gather group) of the kernel the call reaches"""
    fam = fm.family_of(c_in, c_out, mode, ws_enabled, rows_16_byte=layout != "view")
    if fam == "ws":
        return fam, 32, fm.WS_GROUP
    tile, tpw, _ = fm.TWO_PHASE[(fm.cin_pad(c_in), c_out, fam)]
    return fam, tile, tpw


def _sizes(c_in, c_out):
    """{n: the modes to run there}: the edge sizes of every instantiation the shape reaches; a deep size runs one mode per kernel form of the instantiation
    that owns it"""
    out = {}
    layout = _layouts(c_in)[0]
    for mode in fm.MODES:
        fam = fm.family_of(c_in, c_out, mode, False, rows_16_byte=layout != "view")
        tile, tpw, cap = fm.TWO_PHASE[(fm.cin_pad(c_in), c_out, fam)]
        sizes = fm.edge_sizes(tile, tpw, cap)
        for n in sizes[:-1]:
            out.setdefault(n, list(fm.MODES))
        form = mode if fam == "mfma" or mode == "f32" else "bf16x3"            # a shape fused_mfma declines runs fused.hip MODE 1 in four of the modes
        deep = out.setdefault(sizes[-1], [])
        if form == mode:
            deep.append(mode)
    return out


def _cases():
    cs = []
    for c_in, c_out in SHAPES:
        for n, modes in sorted(_sizes(c_in, c_out).items()):
            if n > 20000:
                cs.append((c_in, c_out, n, (c_in, c_out) in RAGGED_AT_DEPTH))
            elif n >= 1:
                cs += [(c_in, c_out, n, False), (c_in, c_out, n, True)]
    return cs


class Case:
    """graph, inputs, plan and the fp64 reference of one (shape, n, graph kind)"""

    def __init__(self, c_in, c_out, n, ragged, seed=0):
        from dgnn_amd import ops
        self.c_in, self.c_out, self.n, self.ragged, self.n_src = c_in, c_out, n, ragged, n + 37
        g = (fm.ragged_graph if ragged else fm.regular_graph)(n, self.n_src, 100 * c_in + c_out + n + seed)
        self.ei = torch.from_numpy(g)
        self.deg = fm.in_degrees(g, n)
        self.inp = fm.layer_inputs(c_in, c_out, self.n_src, self.ei.size(1), n + c_in + c_out + seed)
        self.x, self.ea = self.inp[0], self.inp[1]
        self.par = [t.to(DEV) for t in self.inp[2:]]                       # We, be, Wj, bj, Wi, scale, shift
        self.ea_d = self.ea.to(DEV)
        self.rowptr, self.src, self.eid = ops.plan_build(self.ei.to(DEV), n, 1, n_other=self.n_src)
        self.rows = {}

    def reference(self, **kw):
        We, be, Wj, bj, Wi, scale, shift = self.inp[2:]
        a = dict(bj=bj, scale=scale, shift=shift, relu=True)
        a.update(kw)
        return fm.reference(self.x, self.ea, self.ei, self.n, We, be, Wj, a["bj"], Wi, a["scale"], a["shift"], relu=a["relu"])

    def xs(self, layout):
        if layout not in self.rows:
            self.rows[layout] = _rows(self.x, layout)
        return self.rows[layout]

    def run(self, mode, layout, rng=None, out=None, plan_order=False, prepared=None, bj=True, affine=True, relu=True):
        from dgnn_amd import ops
        We, be, Wj, bj_, Wi, scale, shift = self.par
        xs = self.xs(layout)
        b, e = rng if rng is not None else (0, self.n)
        ea, eid = self.ea_d, self.eid
        if plan_order and eid is not None:
            ea, eid = self.ea_d[eid.long()], None
        return ops.sage_layer_fused_fwd(self.rowptr[b:e + 1], self.src, e - b, xs, ea, We, be, Wj, bj_ if bj else None, Wi, scale if affine else None,
                                        shift if affine else None, relu, gemm_mode=ops.GEMM_MODE_NAMES[mode], out=out, eid=eid,
                                        x_dst=None if rng is None else xs[b:e], prepared=prepared)


def _assert_inside(what, out, ref, mag, kappa, deg, tpw, key=None):
    worst, rep = fm.check_elements(out.cpu(), ref, BOUND_SCALE * kappa * mag + 1e-30, deg, tpw)
    if key is not None:
        WORST[key] = max(WORST.get(key, 0.0), worst)
    print("%s: err / bound <= %.2e" % (what, worst))
    assert rep is None, (what, rep)
    return worst


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nlargest err / bound per (shape, mode):")
        for key in sorted(WORST, key=str):
            print("  %-40s %.2e" % (" ".join(str(k) for k in key), WORST[key]))


@pytest.mark.parametrize("c_in,c_out,n,ragged", _cases())
def test_every_element_vs_fp64(c_in, c_out, n, ragged):
    modes = _sizes(c_in, c_out)[n]
    ws = _ws_enabled()
    c = Case(c_in, c_out, n, ragged)
    ref, mag = c.reference()
    layouts = _layouts(c_in) if n < 20000 else _layouts(c_in)[:1]
    for layout in layouts:
        for mode in modes:
            fam, tile, tpw = _geometry(c_in, c_out, mode, layout, ws)
            buf = torch.full((n + 2, c_out), NAN, device=DEV)
            out = c.run(mode, layout, out=buf)
            assert out.data_ptr() == buf.data_ptr() and bool(torch.isnan(buf[n:]).all()), "rows behind the result were written"
            _assert_inside("%d->%d n=%d %s %s %s (%s)" % (c_in, c_out, n, "ragged" if ragged else "regular", layout, mode, fam), buf[:n], ref, mag, fm.KAPPA[mode],
                           c.deg, tpw, key=("%d->%d" % (c_in, c_out), mode, fam))


def _cuts(tile, tpw):
    return sorted(set(range(1, 8)) | {tpw, tile - 1, tile + 1})


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("c_in,c_out", SHAPES)
def test_same_bits(c_in, c_out, ragged):
    from dgnn_amd import ops
    ws = _ws_enabled()
    cases = {}
    for mode in fm.MODES:
        layout = _layouts(c_in)[0]
        fam, tile, tpw = _geometry(c_in, c_out, mode, layout, ws)
        if fam == "ws":
            continue                                          # tests/test_gpu_ws.py owns the wave-specialised kernel's repeats and sub-ranges
        n = 9 * tile + 9
        if n not in cases:
            c = Case(c_in, c_out, n, ragged, seed=1)
            cases[n] = (c,) + c.reference()
        c, ref, mag = cases[n]
        what = "%d->%d n=%d %s %s" % (c_in, c_out, n, "ragged" if ragged else "regular", mode)
        out = c.run(mode, layout)
        _assert_inside(what, out, ref, mag, fm.KAPPA[mode], c.deg, tpw)
        for _ in range(3):
            assert torch.equal(out, c.run(mode, layout)), what + ": repeat"
        assert torch.equal(out, c.run(mode, layout, plan_order=True)), what + ": edge rows in plan order"
        other = "contiguous"                                  # (the 28- / 29-column view against a contiguous copy of it)
        assert _geometry(c_in, c_out, mode, other, ws)[0] == fam
        assert torch.equal(out, c.run(mode, other)), what + ": contiguous rows"
        if mode == "f16x2":
            We, be, Wj, _, Wi = c.par[:5]
            prep = ops.sage_layer_prepare(We, be, Wj, Wi)
            assert (prep is not None) == (c_in % (fm.cin_pad(c_in) // 16) == 0), "prepared parameters exist for the shapes fused_mfma.hip takes"
            if prep is not None:
                assert torch.equal(out, c.run(mode, layout, prepared=prep)), what + ": prepared parameters"
                assert torch.equal(out, c.run(mode, layout, prepared=prep, plan_order=True)), what + ": prepared parameters, plan order"
        for cut in _cuts(tile, tpw):
            parts = torch.full((n, c_out), NAN, device=DEV)
            c.run(mode, layout, rng=(0, cut), out=parts[:cut])
            c.run(mode, layout, rng=(cut, n), out=parts[cut:])
            if not ragged:
                assert torch.equal(parts, out), what + ": cut at %d" % cut
            else:
                whole = cut // tpw * tpw
                assert torch.equal(parts[:whole], out[:whole]), what + ": whole groups before the cut at %d" % cut
                _assert_inside(what + " cut at %d" % cut, parts, ref, mag, fm.KAPPA[mode], c.deg, None)


@pytest.mark.parametrize("c_in,c_out", [(48, 128), (96, 128), (28, 64)])
def test_epilogue_switches(c_in, c_out):
    """bias, folded BatchNorm and ReLU are switches of every epilogue: fused.hip's, fused_mfma.hip's full-K one (four waves, cin_pad <= 64) and its K-split one
    (eight waves, cin_pad 128)"""
    ws = _ws_enabled()
    layout = _layouts(c_in)[0]
    n = 9 * 32 + 9
    c = Case(c_in, c_out, n, True, seed=2)
    for name, kw, rkw in [("bj=None", dict(bj=False), dict(bj=None)), ("scale=shift=None", dict(affine=False), dict(scale=None, shift=None)),
                          ("relu=False", dict(relu=False), dict(relu=False)),
                          ("none of the three", dict(bj=False, affine=False, relu=False), dict(bj=None, scale=None, shift=None, relu=False))]:
        ref, mag = c.reference(**rkw)
        for mode in fm.MODES:
            fam, tile, tpw = _geometry(c_in, c_out, mode, layout, ws)
            out = c.run(mode, layout, **kw)
            _assert_inside("%d->%d %s %s (%s)" % (c_in, c_out, name, mode, fam), out, ref, mag, fm.KAPPA[mode], c.deg, tpw)
            if name == "relu=False":
                assert bool((out < 0).any())


DEC_SIZES = [1, 5, 32 * 3 + 9, 9 * 32 + 9, 4 * 256 * 32 + 41]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("n", DEC_SIZES)
@pytest.mark.parametrize("c_in", [72, 96, 128])
def test_two_phase_decoder_launch_vs_fp64(c_in, n, ragged):
    """the last layer's launch that carries the decoder, two-phase form (fused_mfma.hip DEC: TILE 32, four cells per wave, the epilogue transposed, stage D on
    waves 0 and 1): logits of every cell against fp64; prepared parameters, repeats and destination sub-ranges bit for bit"""
    from dgnn_amd import ops
    if ops.GEMM_MODE != ops.GEMM_F16X2 or not ops.FUSE_DECODER:
        pytest.skip("the decoder-carrying launch is the default arithmetic's (DGNN_GEMM_MODE / DGNN_FUSE_DECODER)")
    if c_in == 128 and _ws_enabled():
        pytest.skip("c_in = 128 runs the wave-specialised kernel (tests/test_gpu_ws.py) unless DGNN_WS=0")
    c = Case(c_in, 128, n, ragged, seed=3)
    dec = fm.decoder_inputs(n + c_in)
    ref, mag = c.reference()
    lref, lmag = fm.decoder_reference(ref, mag, *dec)
    dd = [t.to(DEV) for t in dec]
    We, be, Wj, bj, Wi, scale, shift = c.par
    what = "decoder launch %d->128 n=%d %s" % (c_in, n, "ragged" if ragged else "regular")

    def run(layout, rng=None, out=None, prepared=None, plan_order=False):
        xs = c.xs(layout)
        b, e = rng if rng is not None else (0, n)
        ea, eid = c.ea_d, c.eid
        if plan_order and eid is not None:
            ea, eid = c.ea_d[eid.long()], None
        return ops.sage_layer_fused_decoder_fwd(c.rowptr[b:e + 1], c.src, e - b, xs, ea, We, be, Wj, bj, Wi, scale, shift, True, *dd, out=out, eid=eid,
                                                x_dst=None if rng is None else xs[b:e], prepared=prepared)

    buf = torch.full((n + 2, 2), NAN, device=DEV)
    lg = run("padded", out=buf)
    assert bool(torch.isnan(buf[n:]).all()), "rows behind the logits were written"
    lg = buf[:n]
    worst, rep = fm.check_elements(lg.cpu(), lref, BOUND_SCALE * fm.K_LOGIT * lmag + 1e-30, c.deg, 4)
    WORST[("%d->128+decoder" % c_in, "f16x2", "mfma DEC")] = max(WORST.get(("%d->128+decoder" % c_in, "f16x2", "mfma DEC"), 0.0), worst)
    print("%s: err / bound <= %.2e" % (what, worst))
    assert rep is None, (what, rep)
    if n > 20000:
        return
    for _ in range(3):
        assert torch.equal(lg, run("padded")), what + ": repeat"
    assert torch.equal(lg, run("contiguous")), what + ": contiguous rows"
    assert torch.equal(lg, run("padded", plan_order=True)), what + ": edge rows in plan order"
    prep = ops.sage_layer_prepare(We, be, Wj, Wi, decoder=tuple(dd))
    assert prep is not None
    assert torch.equal(lg, run("padded", prepared=prep)), what + ": prepared parameters"
    if n >= 40:
        for cut in _cuts(32, 4):
            parts = torch.full((n, 2), NAN, device=DEV)
            run("padded", rng=(0, cut), out=parts[:cut], prepared=prep if cut & 1 else None)
            run("padded", rng=(cut, n), out=parts[cut:])
            if not ragged:
                assert torch.equal(parts, lg), what + ": cut at %d" % cut
            else:
                whole = cut // 4 * 4
                assert torch.equal(parts[:whole], lg[:whole]), what + ": whole groups before the cut at %d" % cut
                w2, rep2 = fm.check_elements(parts.cpu(), lref, BOUND_SCALE * fm.K_LOGIT * lmag + 1e-30, c.deg, None)
                assert rep2 is None, (what, cut, rep2)
