"""The fp32 streaming kernels that run around the fused layers in every default training step, each against a plain fp64 restatement
(streaming_model.py) at the shapes where such kernels go wrong: the BatchNorm chain of csrc/norm.hip on its scalar and its vectorised route,
dgnn_bn_stats_finalize_fold on partial sums of its own, the two-rank halves of the BatchNorm backward, the one-launch Adam of csrc/adam.hip
across its launch and chunk boundaries, and the ReLU pair / row gather / row scatter of csrc/plan.hip.

fp32 rows are read exactly, so every bound is the fp64 value's own magnitude terms times a small multiple of 2^-23 (the constants of
test_bf16_batchnorm_kernels_edges_vs_fp64 without its bf16 storage term); the row moves and the ReLU pair are exact.  The fp64 side of the
BatchNorm cases is evaluated by torch in float64 on the device (the same plain formulas; a 70 001 x 1024 case is seconds on the host).
The largest observed error / bound of every named bound is printed when the module finishes (pytest -s)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import streaming_model as SM
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

F32 = 2.0 ** -23
MOMENTUM, EPS = 0.1, 1e-5
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for k in sorted(RATIOS):
        print("\n[streaming_f32] max error / bound  %-28s %.3f" % (k, RATIOS[k]), end="")
    print()


def held(name, got, want, bound):
    """|got - want| <= bound element by element (torch or numpy); keeps the largest error / bound per name"""
    if isinstance(got, np.ndarray):
        err = np.abs(np.asarray(got, np.float64) - want)
        if err.size == 0:
            return
        bad = ~(err <= bound)
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        nbad = int(bad.sum())
    else:
        err = (got.double() - want).abs()
        if err.numel() == 0:
            return
        bound = bound.expand_as(err)
        bad = ~(err <= bound)
        one = torch.ones_like(err)
        ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, one), torch.where(err > 0, one * math.inf, one * 0)).max().item()
        nbad = int(bad.sum().item())
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    assert nbad == 0, "%s: %d elements outside the bound, worst error = %.3g x bound" % (name, nbad, ratio)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- a. the fp32 BatchNorm chain ---------------------------------------------------------------------------------------------------
LAYOUTS = ("packed", "padded", "shifted")
MS = (1, 2, 3, 64, 65, 257, 12353, 32768, 70001)      # one block .. rows per block > 64, 193 blocks (the finaliser's unrolled loop), 512 (4 columns per workgroup), the 1024-block cap
CS = (1, 3, 4, 28, 64, 96, 128, 256, 260, 512, 1024)
REDUCED_M, REDUCED_C = (3, 257, 12353), (3, 64, 260)
CHAIN_CASES = sorted({(M, c, l) for M in MS for c in (28, 128) for l in LAYOUTS} | {(M, c, l) for M in REDUCED_M for c in CS for l in LAYOUTS}
                     | {(70001, 1024, "packed")})
# the widths k_colreduce4<., float> takes when every row starts on 16 bytes: a power of two from 4 to 256 (one window) or a multiple of 256
# (512: two blockIdx.y windows, 1024: four); the shifted layout starts 4 bytes off and always takes the scalar k_colreduce
VECTOR_ROUTE = {(c, l) for c in (4, 64, 128, 256, 512, 1024) for l in ("packed", "padded")}


def colreduce4_ok(c):
    V = 4                                                   # 16 bytes of fp32
    return c >= V and ((c <= 64 * V and (c & (c - 1)) == 0) or c % (64 * V) == 0)


def takes_vector_route(c, *rows):
    """launch_colreduce's predicate: the width, and every row matrix 16-byte aligned with a row stride that is a multiple of 4 elements"""
    return colreduce4_ok(c) and all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 for t in rows)


def lay(t, layout):
    """the [M, c] device matrix `t` as packed rows, rows padded to c + 4 (still 16-byte aligned) or the [:, 1:] view of c + 1 wide rows (the
    4-byte misalignment of the scene's feature rows behind their loss-weight column); pads are NaN, nothing may read them"""
    M, c = t.shape
    if layout == "packed":
        return t.contiguous()
    buf = torch.full((M, c + (4 if layout == "padded" else 1)), float("nan"), device=t.device, dtype=t.dtype)
    view = buf[:, :c] if layout == "padded" else buf[:, 1:]
    view.copy_(t)
    return view


def bn_inputs(M, c, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    x = rn(M, c) * 2 + rn(c)
    x[:, 0] = 0.75                                           # constant column: variance exactly 0
    if c > 1:
        x[:, 1] = 1e3 + rn(M)                                # mean 1e3, unit spread: E[x^2] - E[x]^2 in fp32 would lose it
    dy = rn(M, c)
    gamma, beta = torch.rand(c, generator=g, device=DEV) + 0.5, rn(c) * 0.3
    rm0, rv0 = rn(c), torch.rand(c, generator=g, device=DEV) + 0.5
    return x, dy, gamma, beta, rm0, rv0


def check_stats(tag, M, X, mean, var, rm, rv, rm0, rv0):
    m64, v64, erm, erv = SM.bn_stats(X, rm0.double(), rv0.double(), MOMENTUM)
    held(tag + "mean", mean, m64, 2 * F32 * X.abs().max(0).values)
    held(tag + "var", var, v64, 4 * F32 * v64 + 1e-12 * X.pow(2).max(0).values)
    unb = v64 * (M / (M - 1)) if M > 1 else v64
    held(tag + "running_mean", rm, erm, 4 * F32 * (rm0.double().abs() + m64.abs()))
    held(tag + "running_var", rv, erv, 4 * F32 * (rv0.double().abs() + unb))
    return m64, v64


def check_bwd(tag, X, Y, DY, gamma, mean, var, train, relu, dx, dgamma, dbeta, count=None, sums=None):
    r = SM.bn_relu_bwd(X, Y, DY, gamma.double(), mean.double(), var.double(), EPS, train, relu, count=count, sums=sums)
    held(tag + "dbeta", dbeta, r.dbeta, 2 * F32 * r.mag_dbeta)
    held(tag + "dgamma", dgamma, r.dgamma, 8 * F32 * r.mag_dgamma + 1e-30)
    held(tag + "dx", dx, r.dx, 16 * F32 * r.mag_dx)
    return r


@pytest.mark.parametrize("M,c,layout", CHAIN_CASES)
def test_f32_batchnorm_kernels_edges_vs_fp64(M, c, layout):
    """dgnn_bn_batch_stats with the running buffers, dgnn_bn_fold, dgnn_scale_shift_act, dgnn_bn_relu_bwd and dgnn_colsum on fp32 rows against
    fp64 per column / per element: 1 .. 70 001 rows, 1 .. 1024 columns, the three row layouts, a constant column, a mean-1e3 column, the
    unbiased running variance (one row keeps the biased value).  The backward's mask is the kernel's own y.  Which column-reduction kernel a
    (width, layout) takes is restated here and held against the table above."""
    from dgnn_amd import ops
    x, dy, gamma, beta, rm0, rv0 = bn_inputs(M, c, M * 7 + c)
    xg, dyg = lay(x, layout), lay(dy, layout)
    assert (xg.stride(0) != c) == (layout != "packed") or M == 1
    assert takes_vector_route(c, xg) == ((c, layout) in VECTOR_ROUTE), "route table changed: edit VECTOR_ROUTE with it"
    X, DY = xg.double(), dyg.double()
    assert torch.equal(X, x.double())
    rm, rv = rm0.clone(), rv0.clone()
    mean, var = ops.bn_batch_stats(xg, rm, rv, MOMENTUM)
    m64, v64 = check_stats("", M, X, mean, var, rm, rv, rm0, rv0)
    assert var[0].item() == 0.0
    if c > 1:
        assert abs(var[1].item() - v64[1].item()) <= 1e-5 * v64[1].item() + 1e-30
    scale, shift = ops.bn_fold(gamma, beta, mean, var, EPS)
    s64, _ = SM.bn_fold(gamma.double(), beta.double(), m64, v64, EPS)
    held("scale", scale, s64, 8 * F32 * s64.abs())
    y = ops.scale_shift_act(xg, scale, shift, True)
    assert y.dtype == torch.float32 and y.shape == (M, c)
    S, T = scale.double(), shift.double()
    held("y", y, torch.relu(X * S + T), 4 * F32 * (X.abs() * S.abs() + T.abs()))
    yg = lay(y, layout)
    assert takes_vector_route(c, xg, yg, dyg) == ((c, layout) in VECTOR_ROUTE)
    dx, dgamma, dbeta = ops.bn_relu_bwd(xg, yg, dyg, gamma, mean, var, EPS, True, True)
    assert dx.shape == (M, c) and dx.is_contiguous()
    check_bwd("", X, y.double(), DY, gamma, mean, var, True, True, dx, dgamma, dbeta)
    held("colsum", ops.colsum(dyg), DY.sum(0), 2 * F32 * DY.abs().sum(0))


def _raw(fn, *args):
    from dgnn_amd._lib import check, lib, ptr, stream_ptr
    a = [ptr(t) if (t is None or isinstance(t, torch.Tensor)) else t for t in args]
    check(getattr(lib(), fn)(*a, stream_ptr()), fn)


def _scratch(M, c):
    from dgnn_amd._lib import lib
    return torch.empty(int(lib().dgnn_colstats_scratch_elems(M, c)), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("M", REDUCED_M)
@pytest.mark.parametrize("c", REDUCED_C)
def test_f32_batchnorm_variants_vs_fp64(M, c):
    """What the training step's default call leaves out: train=0 (dx = g gamma / sqrt(var + eps), dgamma / dbeta still the sums), relu=0 with no y,
    the one-pass dgnn_bn_batch_stats_fold (the bits of stats + fold), dgnn_colsum's accumulate switch, and ldy / lddx wider than the row"""
    from dgnn_amd import ops
    x, dy, gamma, beta, rm0, rv0 = bn_inputs(M, c, M * 11 + c)
    X, DY = x.double(), dy.double()
    rm, rv = rm0.clone(), rv0.clone()
    mean, var = ops.bn_batch_stats(x, rm, rv, MOMENTUM)
    scale, shift = ops.bn_fold(gamma, beta, mean, var, EPS)
    y = ops.scale_shift_act(x, scale, shift, True)
    # eval-mode backward on the running statistics
    ye = ops.scale_shift_act(x, *ops.bn_fold(gamma, beta, rm, rv, EPS), True)
    dx, dgamma, dbeta = ops.bn_relu_bwd(x, ye, dy, gamma, rm, rv, EPS, False, True)
    check_bwd("eval ", X, ye.double(), DY, gamma, rm, rv, False, True, dx, dgamma, dbeta)
    # no ReLU, no y
    dx, dgamma, dbeta = ops.bn_relu_bwd(x, None, dy, gamma, mean, var, EPS, True, False)
    check_bwd("norelu ", X, None, DY, gamma, mean, var, True, False, dx, dgamma, dbeta)
    dx, dgamma, dbeta = ops.bn_relu_bwd(x, None, dy, gamma, rm, rv, EPS, False, False)
    check_bwd("norelu eval ", X, None, DY, gamma, rm, rv, False, False, dx, dgamma, dbeta)
    # one pass: statistics and fold (k_stats_finalize's fold is the arithmetic of k_bn_fold on the values just stored)
    out = [torch.full((c,), float("nan"), device=DEV) for _ in range(4)]
    rm2, rv2 = rm0.clone(), rv0.clone()
    _raw("dgnn_bn_batch_stats_fold", x, c, M, c, out[0], out[1], rm2, rv2, MOMENTUM, gamma, beta, EPS, out[2], out[3], _scratch(M, c))
    for got, want in zip(out + [rm2, rv2], (mean, var, scale, shift, rm, rv)):
        assert same_bits(got, want)
    # colsum: accumulate=1 adds to what is there, accumulate=0 overwrites whatever is there
    out0 = torch.randn(c, generator=torch.Generator().manual_seed(c)).to(DEV) * 50
    acc = out0.clone()
    _raw("dgnn_colsum", dy, c, M, c, acc, 1, _scratch(M, c))
    held("colsum accumulate", acc, out0.double() + DY.sum(0), 2 * F32 * (out0.double().abs() + DY.abs().sum(0)))
    over = torch.full((c,), float("nan"), device=DEV)
    _raw("dgnn_colsum", dy, c, M, c, over, 0, _scratch(M, c))
    assert same_bits(over, ops.colsum(dy)) and not torch.isnan(over).any()
    # destination rows wider than c: the columns beyond c are not written
    ld = c + 3
    yw = torch.full((M, ld), float("nan"), device=DEV)
    _raw("dgnn_scale_shift_act", x, c, scale, shift, 1, M, c, yw, ld)
    assert same_bits(yw[:, :c], y) and torch.isnan(yw[:, c:]).all()
    dxw = torch.full((M, ld), float("nan"), device=DEV)
    dg2, db2 = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    _raw("dgnn_bn_relu_bwd", x, c, yw, ld, dy, c, gamma, mean, var, EPS, 1, 1, M, c, dxw, ld, dg2, db2, _scratch(M, c))
    assert torch.isnan(dxw[:, c:]).all()           # (ldy = c + 3 sends c = 64 down the scalar route: the sums may differ from the packed call's at an exact tie)
    check_bwd("wide ", X, y.double(), DY, gamma, mean, var, True, True, dxw[:, :c], dg2, db2)


# ---- b. dgnn_bn_stats_finalize_fold on partial sums of its own -----------------------------------------------------------------------
def _partials(nblk, c, seed, rows=32):
    """fp64 [nblk][2][c] = (sum, sum of squares) of `rows` rows per block with a block mean and a block variance >= 0: consistent by construction"""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(c, generator=g, dtype=torch.float64) * 3
    mb = mu + torch.randn(nblk, c, generator=g, dtype=torch.float64) * 0.5
    vb = torch.rand(nblk, c, generator=g, dtype=torch.float64) + 0.1
    return torch.stack([rows * mb, rows * (vb + mb * mb)], 1).contiguous(), rows * nblk


def _finalize(P, M, c, gamma, beta, rm, rv, fold=True):
    mean, var = torch.full((c,), float("nan"), device=DEV), torch.full((c,), float("nan"), device=DEV)
    scale, shift = (torch.full((c,), float("nan"), device=DEV), torch.full((c,), float("nan"), device=DEV)) if fold else (None, None)
    Pd = P.to(DEV)
    _raw("dgnn_bn_stats_finalize_fold", Pd, P.shape[0], M, c, mean, var, rm, rv, MOMENTUM, gamma, beta, EPS, scale, shift)
    torch.cuda.synchronize()
    return mean, var, scale, shift


def _exact_sums(P):
    """the partials' sums without a summation order: math.fsum is exactly rounded"""
    a = P.numpy()
    return (torch.tensor([math.fsum(a[:, q, j]) for j in range(a.shape[2])], dtype=torch.float64, device=DEV) for q in (0, 1))


def check_finalize(tag, P, M, c, mean, var, scale, shift, gamma, beta, rm, rv, rm0, rv0):
    """the bounds of (a) with the rows' magnitudes taken from the sums: max |x| -> the root mean square, max x^2 -> the mean square (both no
    larger).  shift = beta - mean * scale: the product carries the mean's rounding (2^-24), the scale's bound (8 * 2^-23) and its own
    rounding (2^-24), the difference one more of its value."""
    S, Q = _exact_sums(P)
    m64 = S / M
    v64 = (Q / M - m64 * m64).clamp_min(0)
    ms = Q / M
    held(tag + "mean", mean, m64, 2 * F32 * ms.sqrt())
    held(tag + "var", var, v64, 4 * F32 * v64 + 1e-12 * ms)
    unb = v64 * (M / (M - 1)) if M > 1 else v64
    if rm is not None:
        held(tag + "running_mean", rm, (1 - MOMENTUM) * rm0.double() + MOMENTUM * m64, 4 * F32 * (rm0.double().abs() + m64.abs()))
        held(tag + "running_var", rv, (1 - MOMENTUM) * rv0.double() + MOMENTUM * unb, 4 * F32 * (rv0.double().abs() + unb))
    if scale is not None:
        s64, t64 = SM.bn_fold(None if gamma is None else gamma.double(), None if beta is None else beta.double(), m64, v64, EPS)
        held(tag + "scale", scale, s64, 8 * F32 * s64.abs())
        held(tag + "shift", shift, t64, 9 * F32 * (m64 * s64).abs() + F32 * t64.abs())


@pytest.mark.parametrize("nblk", [1, 63, 64, 65, 193, 511, 512, 769, 1025, 4400])
@pytest.mark.parametrize("c", [1, 5, 16, 17, 64])
def test_bn_stats_finalize_fold_alone_vs_exact_sums(nblk, c):
    """The finaliser the GEMM epilogue's partial rows go through, on partial sums drawn by the host: fewer partial rows than slices, the
    four-at-a-time loop with and without a tail, the switch to 4 columns per workgroup at 512 partial rows with widths that are no multiple of
    4 or 16, 4 400 partial rows (a 140k-cell layer); with and without gamma / beta / running buffers / the fold"""
    P, M = _partials(nblk, c, nblk * 131 + c)
    g = torch.Generator().manual_seed(c)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(DEV), (torch.randn(c, generator=g) * 0.3).to(DEV)
    rm0, rv0 = torch.randn(c, generator=g).to(DEV), (torch.rand(c, generator=g) + 0.5).to(DEV)
    rm, rv = rm0.clone(), rv0.clone()
    mean, var, scale, shift = _finalize(P, M, c, gamma, beta, rm, rv)
    check_finalize("finalize ", P, M, c, mean, var, scale, shift, gamma, beta, rm, rv, rm0, rv0)
    # no affine parameters, no running buffers: scale = 1 / sqrt(var + eps), shift = -mean * scale
    mean2, var2, scale2, shift2 = _finalize(P, M, c, None, None, None, None)
    assert same_bits(mean2, mean) and same_bits(var2, var)
    check_finalize("finalize ", P, M, c, mean2, var2, scale2, shift2, None, None, None, None, None, None)
    # no fold either: mean and var alone
    mean3, var3, _, _ = _finalize(P, M, c, None, None, None, None, fold=False)
    assert same_bits(mean3, mean) and same_bits(var3, var)


@pytest.mark.parametrize("c", [1, 5, 64])
def test_bn_stats_finalize_fold_of_one_row_keeps_the_biased_variance(c):
    g = torch.Generator().manual_seed(c)
    x = (torch.randn(c, generator=g) * 3).double()                 # fp32 values: x * x is exact in fp64
    P = torch.stack([x, x * x], 0)[None].contiguous()
    rm0, rv0 = torch.randn(c, generator=g).to(DEV), (torch.rand(c, generator=g) + 0.5).to(DEV)
    rm, rv = rm0.clone(), rv0.clone()
    mean, var, scale, shift = _finalize(P, 1, c, None, None, rm, rv)
    check_finalize("finalize ", P, 1, c, mean, var, scale, shift, None, None, rm, rv, rm0, rv0)
    assert torch.equal(var, torch.zeros(c, device=DEV)) and torch.equal(mean.double().cpu(), x)
    held("finalize running_var", rv, (1 - MOMENTUM) * rv0.double(), 4 * F32 * rv0.double())


# ---- c. the two-rank halves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", REDUCED_M)
@pytest.mark.parametrize("c", REDUCED_C)
def test_bn_relu_bwd_two_rank_halves_vs_fp64(M, c):
    """ops.bn_relu_bwd_sums per part of the rows, the parts' sums added in fp64 as functional._SceneBatchNormRelu's all-reduce adds them, then
    ops.bn_relu_bwd_apply per part with count = M: the concatenated dx and the summed sums against the model on the whole matrix, with the
    bounds of the one-piece kernel.  One part that is the whole gives the bits of dgnn_bn_relu_bwd's (dbeta, dgamma); dx may differ in the
    last place there (1.0f / (float)M against (float)(1.0 / count))."""
    from dgnn_amd import ops
    x, dy, gamma, beta, rm0, rv0 = bn_inputs(M, c, M * 13 + c)
    X, DY = x.double(), dy.double()
    mean, var = ops.bn_batch_stats(x)
    y = ops.scale_shift_act(x, *ops.bn_fold(gamma, beta, mean, var, EPS), True)
    dx1, dgamma1, dbeta1 = ops.bn_relu_bwd(x, y, dy, gamma, mean, var, EPS, True, True)
    cuts = sorted({1, M // 3, M})
    for cut in cuts:
        parts = [(a, b) for a, b in ((0, cut), (cut, M)) if b > a]                       # (a rank without rows skips both calls)
        loc = [ops.bn_relu_bwd_sums(x[a:b], y[a:b], dy[a:b], mean, var, EPS, True) for a, b in parts]
        assert all(s.shape == (2, c) and s.dtype == torch.float32 for s in loc)
        glob = sum(s.double() for s in loc).float()
        dx = torch.cat([ops.bn_relu_bwd_apply(x[a:b], y[a:b], dy[a:b], gamma, mean, var, EPS, True, glob, M) for a, b in parts])
        check_bwd("two-rank ", X, y.double(), DY, gamma, mean, var, True, True, dx, glob[1], glob[0])
        if cut == M:
            assert same_bits(glob[0], dbeta1) and same_bits(glob[1], dgamma1)
    # count larger than the local rows and sums that are not the local ones: dx follows the sums and the count it is given
    half = max(1, M // 2)
    sums = torch.randn(2, c, generator=torch.Generator().manual_seed(M)).to(DEV) * M
    dx = ops.bn_relu_bwd_apply(x[:half], y[:half], dy[:half], gamma, mean, var, EPS, True, sums, 3 * M)
    r = SM.bn_relu_bwd(X[:half], y[:half].double(), DY[:half], gamma.double(), mean.double(), var.double(), EPS, True, True, count=3 * M,
                       sums=(sums[0].double(), sums[1].double()))
    held("two-rank dx", dx, r.dx, 16 * F32 * r.mag_dx)


# ---- d. Adam ------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24            # one rounded fp32 operation, relative
ETA = 2.0 ** -149         # ... and absolute where its result is subnormal
LR, B1, B2, AEPS = (float(np.float32(a)) for a in (1e-3, 0.9, 0.999, 1e-8))      # the hyper-parameters as the launch reads them (fp32 arguments)
ADAM_SIZES = (0, 1, 2047, 2048, 2049, 300001)


def gam(k):
    return k * U / (1 - k * U)


def adam_bound(p, g, m, v, t):
    """|fp32 step - fp64 step| from the rounded operations of k_adam, each (1 + d), |d| <= 2^-24 (Higham's gamma_k = k u / (1 - k u) for k of
    them in a product); inputs fp32 values, so the first operation of every chain is the only error there.

      m' = m + (g - m) * w1          sub, the rounding of w1 = 1 - b1, mul: gamma_3 on e = (g - m) w1; the add: u (|m| + |e|)
                                     => dm <= gamma_1 |m| + gamma_4 |g - m| w1
      v' = b2 * v + w2 * g * g       mul, add: gamma_2 on b2 v; w2's rounding, two muls, add: gamma_4 on w2 g g; the three products may be
                                     subnormal (|g| is 1e-12 times a normal deviate: only its tail gets there): eta each       => dv <= gamma_2 b2 v + gamma_4 w2 g g + 3 eta  (<= gamma_4 v' + 3 eta)
      denom = sqrt(v') * c2 + eps    sqrt of a value off by gamma_4 (relative; |sqrt a - sqrt b| <= sqrt |a - b| for the eta part), its own
                                     rounding, c2 rounded once on the host, mul, add: gamma_8 denom + 2 c2 sqrt(3 eta)  =: dd, rd = dd / denom
      q = m' / denom                 => dq <= (|m'| (rd + u + rd u) + dm (1 + u)) / (denom (1 - rd))
      r = c1 * q                     c1 rounded once on the host, mul: |r~ - c1 q| <= c1 (dq (1 + gamma_2) + |q| gamma_2) + eta
      p' = p - r                     => dp <= u |p'| + (1 + u) |r~ - c1 q|
    -> (fp64 p', m', v', dp, dm, dv).  No constant is fitted.  The observed error comes within a percent of dp and dm: where the step is far
    below the value (|r| << |p|, |e| << |m|) the last addition's rounding is all there is, and one rounding reaches 2^-24 of a value just
    above a power of two -- the u |p'| and gamma_1 |m| terms are attained, never passed."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    p64, m64, v64 = SM.adam_step(p, g, m, v, LR, B1, B2, AEPS, t)
    c1, c2 = LR / (1 - math.pow(B1, t)), 1 / math.sqrt(1 - math.pow(B2, t))
    dm = gam(1) * np.abs(m) + gam(4) * np.abs(g - m) * (1 - B1)
    dv = gam(2) * B2 * v + gam(4) * (1 - B2) * g * g + 3 * ETA
    denom = np.sqrt(v64) * c2 + AEPS
    rd = (gam(8) * denom + 2 * c2 * math.sqrt(3 * ETA)) / denom
    q = np.abs(m64) / denom
    dq = (np.abs(m64) * (rd + U + rd * U) + dm * (1 + U)) / (denom * (1 - rd))
    dp = U * np.abs(p64) + (1 + U) * (c1 * (dq * (1 + gam(2)) + q * gam(2)) + ETA)
    return p64, m64, v64, dp, dm, dv


def check_adam_step(before, grads, after, t):
    """every tensor of the group, from the same fp32 state (no drift): the fp64 rule within adam_bound, and the bits of the fp32 restatement
    (the library is built with -ffp-contract=off and without fast-math; HIP's fp32 division and square root are correctly rounded)"""
    for i, ((p0, m0, v0), g, (p1, m1, v1)) in enumerate(zip(before, grads, after)):
        assert p1.shape == p0.shape and p1.dtype == np.float32
        p64, m64, v64, dp, dm, dv = adam_bound(p0, g, m0, v0, t)
        held("adam m", m1, m64, dm)
        held("adam v", v1, v64, dv)
        held("adam p", p1, p64, dp)
        p32, m32, v32 = SM.adam_step_f32(p0, g, m0, v0, LR, B1, B2, AEPS, t)
        for k, a, b in (("p", p1, p32), ("m", m1, m32), ("v", v1, v32)):
            assert np.array_equal(a, b), "tensor %d (%d elements), step %d: %s differs from the fp32 restatement in %d elements" % (
                i, p0.size, t, k, int((a != b).sum()))


def adam_sizes(n):
    s = [ADAM_SIZES[(3 * i + 1) % 5] for i in range(n)]         # the five small sizes in turn
    s[50 if n > 50 else n // 2] = 300001
    for i, v in ((46, 2049), (47, 0), (48, 2049), (49, 0), (94, 0), (95, 2049), (96, 0)):       # 0 and 2049 elements on both sides of a launch boundary (48 | 48 | 1)
        if i < n:
            s[i] = v
    return s


def adam_grads(sizes, step, seed):
    """magnitudes from 1e-12 to 1e6 across the group; tensor n // 3 (the only one: tensor 0 on even steps) gets an all-zero gradient"""
    n = len(sizes)
    g = torch.Generator().manual_seed(seed * 100 + step)
    out = []
    for i, k in enumerate(sizes):
        mag = 10.0 ** (-12 + 18 * i / max(n - 1, 1)) if n > 1 else 1.0
        gr = torch.randn(k, generator=g) * mag
        if i == n // 3 and (n > 1 or step % 2 == 0):
            gr.zero_()
        out.append(gr)
    return out


def _np(t):
    return t.detach().cpu().numpy().copy()


def _snapshot(opt, params):
    return [(_np(p), _np(opt.state[p]["exp_avg"]) if len(opt.state[p]) else np.zeros(p.shape, np.float32),
             _np(opt.state[p]["exp_avg_sq"]) if len(opt.state[p]) else np.zeros(p.shape, np.float32)) for p in params]


@pytest.mark.parametrize("n", [1, 48, 49, 97])
def test_adam_launch_and_chunk_edges_vs_fp64(n):
    """dgnn_amd.optim.Adam over one launch, one full launch (48 tensors), two and three: 0 / 1 / 2047 / 2048 / 2049 / 300 001 elements with the
    empty and the 2049-element tensor on both sides of a launch boundary, gradients from 1e-12 to 1e6 and an all-zero one, steps 1 .. 5; every
    tensor after every step against the fp64 rule from the same state and against the fp32 restatement bit for bit.  An empty tensor has no
    address: the launch must take it and must not shift its neighbours' blocks."""
    from dgnn_amd.optim import Adam
    sizes = adam_sizes(n)
    assert 300001 in sizes and (n < 48 or sizes[47] == 0) and (n < 49 or sizes[48] == 2049) and (n < 97 or (sizes[95], sizes[96]) == (2049, 0))
    g = torch.Generator().manual_seed(n)
    params = [torch.nn.Parameter(torch.randn(k, generator=g).to(DEV)) for k in sizes]
    opt = Adam(params, lr=LR, betas=(B1, B2), eps=AEPS)
    for t in range(1, 6):
        before = _snapshot(opt, params)
        grads = adam_grads(sizes, t, n)
        for p, gr in zip(params, grads):
            p.grad = gr.to(DEV)
        opt.step()
        torch.cuda.synchronize()
        assert all(opt.state[p]["step"] == t for p in params)
        check_adam_step(before, [gr.numpy() for gr in grads], _snapshot(opt, params), t)


def test_adam_late_step_from_a_loaded_state_vs_fp64():
    """t = 10 000 (bias corrections 1 - 0.9^t = 1 exactly in double, 1 - 0.999^t = 1 - 4.5e-5) with the moments and the step count injected through
    load_state_dict, over a launch boundary"""
    from dgnn_amd.optim import Adam
    sizes = adam_sizes(49)
    g = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(k, generator=g).to(DEV)) for k in sizes]
    opt = Adam(params, lr=LR, betas=(B1, B2), eps=AEPS)
    grads = adam_grads(sizes, 1, 5)
    sd = opt.state_dict()
    sd["state"] = {i: {"step": torch.tensor(9999.0), "exp_avg": gr * 0.7 + torch.randn(k, generator=g) * gr.abs().max().item() * 0.1 if k else gr.clone(),
                       "exp_avg_sq": (gr * gr) * 1.3 + 1e-30} for i, (k, gr) in enumerate(zip(sizes, grads))}
    opt.load_state_dict(sd)
    assert all(opt.state[p]["step"] == 9999 for p in params)
    before = _snapshot(opt, params)
    for i, (m0, gr) in enumerate(zip(before, grads)):
        assert np.array_equal(m0[1], sd["state"][i]["exp_avg"].numpy()) and np.array_equal(m0[2], sd["state"][i]["exp_avg_sq"].numpy())
    for p, gr in zip(params, grads):
        p.grad = gr.to(DEV)
    opt.step()
    torch.cuda.synchronize()
    assert all(opt.state[p]["step"] == 10000 for p in params)
    check_adam_step(before, [gr.numpy() for gr in grads], _snapshot(opt, params), 10000)


def test_adam_raw_tables_touch_only_their_tensors():
    """lib().dgnn_adam_step on tables of its own: 50 tensors that are slices of four flat buffers with NaN guard elements between them (a block that
    walked into a neighbour, or past a tensor's end inside its last 2048-element chunk, would write a guard), empty tensors given as NULL
    and as a real address; n_tensors = 0 with NULL tables is a valid call that launches nothing"""
    from dgnn_amd._lib import check, lib, stream_ptr
    L = lib()
    check(L.dgnn_adam_step(0, None, None, None, None, None, LR, B1, B2, AEPS, 1, stream_ptr()), "dgnn_adam_step")
    sizes = [ADAM_SIZES[(2 * i + 3) % 5] for i in range(50)]
    sizes[0], sizes[47], sizes[48], sizes[49] = 0, 2049, 0, 2047
    GUARD = 3
    off, offs = GUARD, []
    for k in sizes:
        offs.append(off)
        off += k + GUARD
    g = torch.Generator().manual_seed(9)
    flat = {}
    for name in "pgmv":
        f = torch.full((off,), float("nan"))
        for o, k in zip(offs, sizes):
            f[o:o + k] = torch.randn(k, generator=g).abs() * 1e-3 if name == "v" else torch.randn(k, generator=g) * (1e-2 if name in "gm" else 1.0)
        flat[name] = f.to(DEV)
    host = {k: v.cpu().numpy().copy() for k, v in flat.items()}
    n = len(sizes)

    def table(name):
        base = flat[name].data_ptr()
        return (C.c_void_p * n)(*[None if (k == 0 and i % 2 == 0) else base + 4 * o for i, (o, k) in enumerate(zip(offs, sizes))])

    t = 4
    check(L.dgnn_adam_step(n, table("p"), table("g"), table("m"), table("v"), (C.c_int64 * n)(*sizes), LR, B1, B2, AEPS, t, stream_ptr()), "dgnn_adam_step")
    torch.cuda.synchronize()
    after = {k: v.cpu().numpy() for k, v in flat.items()}
    sl = [slice(o, o + k) for o, k in zip(offs, sizes)]
    check_adam_step([(host["p"][s], host["m"][s], host["v"][s]) for s in sl], [host["g"][s] for s in sl],
                    [(after["p"][s], after["m"][s], after["v"][s]) for s in sl], t)
    inside = np.zeros(off, bool)
    for s in sl:
        inside[s] = True
    for name in "pgmv":
        assert np.isnan(after[name][~inside]).all(), "a guard element of the %s buffer was written" % name
    assert np.array_equal(after["g"][inside], host["g"][inside])


# ---- e. the ReLU pair and the row moves: exact -------------------------------------------------------------------------------------------
def _sweep():
    """elements of one capped grid sweep of a grid-stride kernel (dgnn_grid_cap: 8 blocks per CU x 256 threads, 256 CUs in the library's table)"""
    return 8 * max(256, torch.cuda.get_device_properties(DEV).multi_processor_count) * 256


def _specials(dtype):
    tiny = torch.tensor([1], dtype=torch.int32 if dtype == torch.float32 else torch.int16).view(dtype)       # the smallest subnormal
    return torch.cat([torch.tensor([-0.0, 0.0, float("inf"), float("-inf")], dtype=dtype), tiny, -tiny])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [0, 1, 255, 257, "sweep"])
def test_relu_pair_is_exact(dtype, n):
    """ops.relu equals torch.relu as values (-0.0 and +0.0 are one value) and ops.relu_bwd passes g exactly where y > 0 and gives zero elsewhere:
    signed zeros, the smallest subnormals (kept, not flushed), infinities, sizes around a block and beyond one capped grid sweep"""
    from dgnn_amd import ops
    n = 2 * _sweep() + 77 if n == "sweep" else n
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g).to(dtype)
    sp = _specials(dtype)
    k = min(n, sp.numel())
    if k:
        x[torch.randperm(n, generator=g)[:k]] = sp[:k]
    if n > 300:
        x[-sp.numel():] = sp                                  # and in the last, partial sweep
    gr = torch.randn(n, generator=g).to(dtype)
    xd, gd = x.to(DEV), gr.to(DEV)
    y = ops.relu(xd)
    assert y.dtype == dtype and y.shape == x.shape and torch.equal(y.cpu(), torch.relu(x))
    assert not (y.cpu() != 0)[x <= 0].any() and same_bits(y.cpu()[x > 0].float(), x[x > 0].float())
    for mask_src in (y, xd):                                  # y of the forward, and any tensor as y (negative values, -inf, -tiny)
        d = ops.relu_bwd(mask_src, gd)
        assert d.dtype == dtype and d.shape == x.shape
        want = torch.where(mask_src.cpu() > 0, gr, torch.zeros_like(gr))
        assert torch.equal(d.cpu(), want) and same_bits(d.cpu()[mask_src.cpu() > 0].float(), gr[mask_src.cpu() > 0].float())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_relu_pair_agrees_on_nan(dtype):
    """NaN is outside torch.relu's contract here: k_relu is fmaxf(x, 0), which drops a NaN operand and stores 0, and k_relu_bwd's y > 0 is false for
    it, so the gradient is blocked.  Asserted is only that the two agree: the gradient passes exactly where the forward kept the value."""
    from dgnn_amd import ops
    x = torch.tensor([1.5, float("nan"), -2.0, float("nan"), 0.25] * 60, dtype=dtype)
    gr = torch.arange(1, x.numel() + 1).to(dtype)
    y = ops.relu(x.to(DEV))
    d = ops.relu_bwd(y, gr.to(DEV)).cpu()
    nan = torch.isnan(x)
    kept = torch.isnan(y.cpu())[nan]                          # the forward kept the NaN
    passed = (d == gr)[nan]
    assert torch.equal(kept, passed)
    assert torch.equal(y.cpu()[~nan], torch.relu(x)[~nan]) and torch.equal(d[~nan], torch.where(x > 0, gr, torch.zeros_like(gr))[~nan])


def _rows(n, w, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int16:
        return torch.randint(-32768, 32767, (n, w), generator=g, dtype=torch.int16)
    t = torch.randn(n, w, generator=g).to(dtype)
    if dtype == torch.float32 and n:
        t.view(torch.int32)[0, 0] = 0x7FC01234                # a NaN with a payload and a negative zero: a bit copy keeps them
        t[-1, -1] = -0.0
    return t


def _bits_any(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _index_lists(n_src, big):
    g = torch.Generator().manual_seed(n_src)
    return {"repeated": torch.tensor([0, n_src - 1, 0, 0, n_src - 1, n_src // 2] * 7), "descending": torch.arange(n_src - 1, -1, -1),
            "random beyond one sweep": torch.randint(0, n_src, (big,), generator=g), "empty": torch.zeros(0, dtype=torch.int64)}


def test_gather_rows_is_a_bit_copy():
    """ops.gather_rows = src[idx, :cols] bit for bit: fewer columns than the row has, padded rows, the [:, 1:] view, repeated / descending / empty
    index lists, more elements than one capped grid sweep; bf16 and int16 rows of even width move as fp32 words, odd widths and strided
    16-bit rows raise"""
    from dgnn_amd import ops
    n_src, w = 501, 40
    lists = _index_lists(n_src, _sweep() // 20 + 13)
    base = _rows(n_src, w + 4, torch.float32, 1).to(DEV)
    sources = {"packed": base[:, :w].contiguous(), "padded": base[:, :w], "shifted": base[:, 1:w + 1]}
    assert sources["padded"].stride(0) == w + 4 and sources["shifted"].data_ptr() % 16 == 4
    for lname, idx in lists.items():
        for sname, src in sources.items():
            for cols in (None, w, 7, 1):
                out = ops.gather_rows(src, idx.to(torch.int32).to(DEV), cols)
                want = src[idx.to(DEV), :cols]
                assert out.is_contiguous() and out.shape == want.shape == (idx.numel(), cols or w), (lname, sname, cols)
                assert same_bits(out, want), (lname, sname, cols)
    for dtype in (torch.bfloat16, torch.int16):
        src = _rows(n_src, 28, dtype, 2).to(DEV)
        for lname, idx in lists.items():
            for cols in (None, 28, 6, 2):
                out = ops.gather_rows(src, idx.to(torch.int32).to(DEV), cols)
                want = src[idx.to(DEV), :cols]
                assert out.dtype == dtype and out.shape == want.shape and torch.equal(_bits_any(out), _bits_any(want)), (dtype, lname, cols)
        i3 = torch.arange(3, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError):
            ops.gather_rows(_rows(9, 27, dtype, 3).to(DEV), i3)                      # odd width
        with pytest.raises(ValueError):
            ops.gather_rows(src, i3, 5)                                              # odd column count
        with pytest.raises(ValueError):
            ops.gather_rows(src[:, :26], i3)                                         # rows that are not contiguous
    with pytest.raises(ValueError):
        ops.gather_rows(sources["packed"], torch.arange(3, dtype=torch.int32, device=DEV), w + 1)
    with pytest.raises(ValueError):
        ops.gather_rows(sources["packed"], torch.arange(3, dtype=torch.int32, device=DEV), 0)


def test_scatter_rows_writes_exactly_the_named_rows_and_columns():
    """ops.scatter_rows_(out, idx, src) = `out[idx] = src` bit for bit into NaN-filled strided rows: only the rows idx names and only src's columns
    change (the pads around `out`, and its columns beyond src's width, stay as they were); source rows of another stride than the
    destination's; an empty index list; more elements than one capped grid sweep; bf16 / int16 rows as fp32 words"""
    from dgnn_amd import ops
    NANBITS = 0x7FC00AAA
    for n_out, w, n in ((300, 40, 120), (70000, 24, _sweep() // 24 + 5), (50, 1, 50), (50, 9, 0)):
        g = torch.Generator().manual_seed(n_out + w)
        idx = torch.randperm(n_out, generator=g)[:n]                                 # distinct rows (two writers of one row would race), any order
        for src_pad, out_lo, out_hi, w_out in ((0, 0, 0, w), (0, 1, 2, w), (0, 2, 0, w + 3), (5, 1, 2, w), (2, 0, 0, w)):
            srcbuf = _rows(n, w + src_pad, torch.float32, n + src_pad).to(DEV)
            src = srcbuf[:, :w]
            buf = torch.full((n_out, out_lo + w_out + out_hi), NANBITS, dtype=torch.int32, device=DEV).view(torch.float32)
            out = buf[:, out_lo:out_lo + w_out]
            want = buf.clone()
            want[idx.to(DEV), out_lo:out_lo + w] = src
            ret = ops.scatter_rows_(out, idx.to(DEV), src)
            assert ret is out and same_bits(buf, want), (n_out, w, n, src_pad, out_lo, out_hi, w_out)
    for dtype in (torch.bfloat16, torch.int16):
        n_out, w, n = 200, 28, 77
        idx = torch.randperm(n_out, generator=torch.Generator().manual_seed(4))[:n].to(DEV)
        for ix in (idx, idx[:0]):
            src = _rows(ix.numel(), w, dtype, 6).to(DEV)
            out = _rows(n_out, w, dtype, 7).to(DEV)
            want = out.clone()
            want[ix] = src
            ops.scatter_rows_(out, ix, src)
            assert torch.equal(_bits_any(out), _bits_any(want))
        with pytest.raises(ValueError):
            ops.scatter_rows_(_rows(n_out, 27, dtype, 8).to(DEV), idx[:3], _rows(3, 27, dtype, 9).to(DEV))       # odd width
        with pytest.raises(ValueError):
            ops.scatter_rows_(_rows(n_out, 30, dtype, 8).to(DEV)[:, :28], idx[:3], _rows(3, 28, dtype, 9).to(DEV))   # strided destination
