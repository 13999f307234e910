"""CPU-side model of the fused decoder (dgnn_amd/csrc/decoder.hip, k_decoder_rows_bf16 in fused_bf16.hip) and of the KL cell loss
(dgnn_amd/csrc/loss.hip) for tests/test_decoder_loss_model_cpu.py and tests/test_gpu_decoder_loss_edges.py: fp64 references with the
magnitudes their error bounds are stated in, the kernels' operand splits restated in torch, and inputs whose results are exact in every
summation order.  No GPU import; every function works on the device of its arguments.  gemm_model.py has the shared pieces (embed,
outside_intact, ints, pow2, three_part, bf16_round, ref_fwd, C_FWD_F32, C_FWD_BF16).

Decoder exactness.  `exact_decoder` draws y, W0, b0, W3 from {-3..3} \\ {0}, scale from +-{1/2, 1, 2}, shift and b3 integers: the hidden
layer is a multiple of 1/2 below 128 * 9 * 2 + 6, the projection a multiple of 1/2 below 10^6 -- far below 2^24 halves, so every order of
summation and every split into bf16 parts gives the fp64 logits bit for bit.  `parts_decoder` puts 18-bit (three-part) or 16-bit (two-part)
values in few enough places that all sums stay exact as well; there the proof is test_decoder_loss_model_cpu.py, which evaluates them
sequentially in fp32 and checks the sum of all magnitudes against 2^24 units.

Loss exactness.  `saturated_rows`: targets (1,0) / (0,1), logits an integer d in [128, 512] apart, integer volumes, norm 0: expf(-d) = 0 and
logf(1) = 0, so a row's cell term is exactly 0 or d and the three sums are integers.
"""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn.functional as F

import gemm_model as gm

K_IN, HID = 128, 64
BF16_SINGLE, BF16_COMPENSATED = 0, 1                       # DGNN_BF16_SINGLE / DGNN_BF16_COMPENSATED of include/dgnn_hip.h

# ---- decoder: the kernels ---------------------------------------------------------------------------------------------------------------------
# rows: k_decoder_rows (16-byte aligned rows, stride a multiple of 4); fused_misaligned / fused_stride: k_decoder_fused, reached by a base 4
# bytes off and by an aligned base with a stride that is no multiple of 4; bf16_single / bf16_comp: k_decoder_rows_bf16<128, 0 / 1>
DECODER_KERNELS = ("rows", "fused_misaligned", "fused_stride", "bf16_single", "bf16_comp")
# every edge of the 32- and 64-row tiles, a multi-block size, and the smallest M at which the prefetch branch of both row kernels (more than
# 8 * 256 tiles of 32 rows) and the grid-stride loop of k_decoder_fused (more than 512 tiles of 64) are all taken
DECODER_M = (1, 31, 32, 33, 63, 64, 65, 255, 257, 4097)
DECODER_M_BIG = 65536 + 8 * 32 + 5

Opt = namedtuple("Opt", "n_out b0 ss b3 ldo")               # has b0, has scale / shift, has b3; ldo in {n_out, 3}
ALL_OPTS = tuple(Opt(n, b0, ss, b3, ldo) for n in (1, 2) for b0 in (True, False) for ss in (True, False) for b3 in (True, False)
                 for ldo in sorted({n, 3}))
# each branch both ways, n_out = 1 with ldo = 3 among them: the large M and the range tests
FEW_OPTS = (Opt(1, True, True, True, 3), Opt(2, False, False, False, 2), Opt(1, False, True, False, 1), Opt(2, True, False, True, 3))


def is_bf16(kernel):
    return kernel.startswith("bf16")


def bf16_mode(kernel):
    return BF16_COMPENSATED if kernel == "bf16_comp" else BF16_SINGLE


# ---- decoder: the operand splits of csrc/fused_common.h (split3) and csrc/fused_bf16.hip (split2), restated -----------------------------------
def split2(x):
    """(hi, lo): hi = bf16(x), lo = bf16(x - hi), both as fp32; x = hi + lo to 16 bits"""
    hi = gm.bf16_round(x)
    return hi, gm.bf16_round(x - hi)


def split3(x):
    """(hi, mid, lo), each a bf16 value as fp32, rounding to nearest at every step; x = hi + mid + lo exactly (24 bits)"""
    hi = gm.bf16_round(x)
    mid = gm.bf16_round(x - hi)
    return hi, mid, gm.bf16_round(x - hi - mid)


def w0_as_seen(W0, kernel):
    """W0 as the kernel's matrix products see it: fp32 kernels all 24 bits, the bf16 decoder hi + lo (compensated) or hi alone (single)"""
    if not is_bf16(kernel):
        return W0.double()
    hi, lo = split2(W0.float())
    return hi.double() + lo.double() if kernel == "bf16_comp" else hi.double()


# ---- decoder: the fp64 reference ------------------------------------------------------------------------------------------------------------------
def ref_decoder(y, W0, b0, scale, shift, W3, b3):
    """(logits, magnitude) in fp64.  logits = W3 relu((W0 y + b0) scale + shift) + b3; absent b0 / scale, shift / b3 are 0 / 1, 0 / 0.
    magnitude = |W3| m1 + |W3| h + |b3| summed over the hidden channels, m1 = (|y||W0|^T + |b0|)|scale| + |shift| the magnitude of the first
    stage and h its fp64 result after the ReLU: the ReLU is 1-Lipschitz, so the first stage's error reaches a logit through |W3|, and the
    projection adds its own rounding on the terms |W3| h and |b3|."""
    assert (scale is None) == (shift is None)
    pre, m1 = gm.ref_fwd(y, W0, bias=b0, scale=scale, shift=shift)
    h = pre.clamp_min(0)
    w3 = W3.double()
    logits, mag = h @ w3.t(), (m1 + h) @ w3.abs().t()
    if b3 is not None:
        logits, mag = logits + b3.double(), mag + b3.double().abs()
    return logits, mag


def seq_decoder_fp32(y, W0, b0, scale, shift, W3, b3):
    """the decoder as plain sequential fp32 sums (rounded product, rounded add): the longest chain an fp32 kernel could run"""
    h = gm.seq_sum_fp32(y.float(), W0.float())
    if b0 is not None:
        h = h + b0.float()
    if scale is not None:
        h = h * scale.float() + shift.float()
    out = gm.seq_sum_fp32(h.clamp_min(0), W3.float())
    return out if b3 is None else out + b3.float()


# ---- decoder: inputs ----------------------------------------------------------------------------------------------------------------------------
DecoderInputs = namedtuple("DecoderInputs", "y W0 b0 scale shift W3 b3")


def with_opts(d, o):
    """the inputs a call with options `o` passes: n_out rows of W3 / b3, None for what is absent"""
    return DecoderInputs(d.y, d.W0, d.b0 if o.b0 else None, d.scale if o.ss else None, d.shift if o.ss else None, d.W3[:o.n_out].contiguous(),
                         d.b3[:o.n_out].contiguous() if o.b3 else None)


def exact_decoder(M, gen, tile_tag=False):
    """integer inputs (module docstring), W3 / b3 for two outputs.  tile_tag: columns 0 and 1 of row r carry its 32-row tile's index in base 61,
    shifted to [-30, 30] (exact in bf16), so rows of different tiles differ in a value the result depends on -- besides the random rest"""
    y = gm.ints((M, K_IN), gen)
    if tile_tag:
        t = torch.arange(M) // 32
        y[:, 0], y[:, 1] = (t % 61 - 30).float(), (t // 61 - 30).float()
        assert y[:, :2].abs().max() <= 30
    return DecoderInputs(y, gm.ints((HID, K_IN), gen), gm.ints((HID,), gen), gm.pow2((HID,), gen, -1, 1), gm.ints((HID,), gen), gm.ints((2, HID), gen),
                         gm.ints((2,), gen))


def range_decoder(M, kind, gen):
    """randn: the shapes of test_decoder_fused.  wide: y and W0 rows over 2^+-8 with elements over 2^+-6 (gemm_model.wide)"""
    if kind == "randn":
        y, W0 = torch.randn(M, K_IN, generator=gen), torch.randn(HID, K_IN, generator=gen) * 0.2
    else:
        y, W0 = gm.wide((M, K_IN), gen, (-8, 8)), gm.wide((HID, K_IN), gen, (-8, 8))
    r = lambda *s: torch.randn(*s, generator=gen)
    return DecoderInputs(y, W0, r(HID), torch.rand(HID, generator=gen) + 0.5, r(HID), r(2, HID) * 0.3, r(2))


def two_part(shape, gen):
    """a + b 2^-8 with a, b from `ints`, drawn again until the bf16 hi and lo parts are both non-zero: 16 significant bits"""
    a, b = gm.ints(shape, gen), gm.ints(shape, gen)
    for _ in range(200):
        v = a + b * 2.0 ** -8
        hi, lo = split2(v)
        bad = (lo == 0) | (hi + lo != v)
        if not bad.any():
            return v
        a, b = (torch.where(bad, gm.ints(shape, gen), t) for t in (a, b))
    raise AssertionError("two_part: no draw with two non-zero parts")


PARTS_COLS = tuple(16 * S + 8 * g + (3 * S + 5 * g) % 8 for S in range(K_IN // 16) for g in range(2))      # one column per k-step and k-group


def _sparse_w3(gen, per_out):
    """[2, HID]: `per_out` entries +-2^e per output (one e in [-1, 1] per output) on channels of both 32-column blocks, zeros elsewhere"""
    W3 = torch.zeros(2, HID)
    for o in range(2):
        ch = torch.cat([torch.randperm(32, generator=gen)[:per_out // 2], 32 + torch.randperm(32, generator=gen)[:per_out - per_out // 2]])
        W3[o, ch] = gm.pow2((1, per_out), gen, -1, 1)[0]
    return W3


def parts_decoder(M, which, gen):
    """Inputs whose result changes if a lower bf16 part of one operand is dropped, and is exact otherwise (no scale / shift).
    which = y3: y holds three-part values in PARTS_COLS -- one column in every 16-wide k-step and both 8-wide k-groups -- and zeros elsewhere,
            W0 is +-1 there; W0_3: the reverse, y +-2^e with one e in [-1, 1] per row; both for k_decoder_rows.
    which = W0_2: W0 holds two-part values in every column against integer y (exact in bf16): for the bf16 decoder, whose compensated mode
            multiplies hi and lo and whose single mode hi alone.
    W3 has 4 (y3, W0_3) or 16 (W0_2) entries +-2^e per output."""
    y, W0 = torch.zeros(M, K_IN), torch.zeros(HID, K_IN)
    cols = list(PARTS_COLS)
    if which == "y3":
        y[:, cols], W0[:, cols] = gm.three_part((M, len(cols)), gen), gm.pow2((HID, len(cols)), gen, 0, 0)
    elif which == "W0_3":
        y[:, cols], W0[:, cols] = gm.pow2((M, len(cols)), gen, -1, 1), gm.three_part((HID, len(cols)), gen)
    else:
        assert which == "W0_2"
        y, W0 = gm.ints((M, K_IN), gen), two_part((HID, K_IN), gen)
    return DecoderInputs(y, W0, gm.ints((HID,), gen), None, None, _sparse_w3(gen, 16 if which == "W0_2" else 4), gm.ints((2,), gen))


def parts_unit(d, which):
    """[M, 2]: the unit every term of logit (r, o) of a parts case is a multiple of -- 2^-16 (2^-8 for two-part values) times the power of two
    of row r of y and of row o of W3.  b0 and b3 are integers and the units at most 1"""
    sy = d.y[:, list(PARTS_COLS)].abs().min(dim=1).values if which == "W0_3" else torch.ones(d.y.size(0))
    s3 = torch.where(d.W3 != 0, d.W3.abs(), torch.full_like(d.W3, float("inf"))).min(dim=1).values
    return (2.0 ** -8 if which == "W0_2" else 2.0 ** -16) * sy[:, None].double() * s3[None, :].double()


def drop_part(x, part):
    """x without its bf16 `part` (mid / lo of split3, lo2 of split2)"""
    if part == "lo2":
        return split2(x)[0]
    hi, mid, lo = split3(x)
    return hi + mid if part == "lo" else hi + lo


# ---- loss: the fp64 reference -------------------------------------------------------------------------------------------------------------------------
NORMS = (0, 1, 2)                                            # regularization.cell_norm: none, log, sqrt (ops.CELL_NORMS)
# every edge of the 64-lane waves and the 1024-row blocks, the limit of the one-launch form and one past it, and the first size at which the
# 256-block grid of k_kl_loss_fwd strides
LOSS_N = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 65536, 65537, 256 * 1024 + 1025)
STEP_MAX_ROWS = 65536

KL = namedtuple("KL", "sum_cw sum_w oa loss dlogits mu w grad_mag grad_tiny cell")
TINY = 2.0 ** -126                                          # the smallest normal fp32 value


def weights64(vol, norm):
    """the volume weights in the reference's form (learning/runModel.py:193-199), in fp64: vol | log(1 + vol) | sqrt(vol)"""
    v = vol.double()
    return torch.log(1 + v) if norm == 1 else (torch.sqrt(v) if norm == 2 else v)


def oa_pred(logits):
    """the reference's class per row (:179), restated: argmax of the fp32 log-softmax pair, (x - max) - log(sum exp(x - max)), first index on a tie"""
    l = logits.float().cpu()
    a = l - l.max(dim=1, keepdim=True).values
    ls = a - torch.log(torch.exp(a).sum(dim=1, keepdim=True))
    return (ls[:, 1] > ls[:, 0]).long()


def ref_kl(logits, gt, vol, norm, grad=1.0):
    """The cell loss in fp64 -> KL: sum_cw = sum_k cell_k w_k, sum_w = sum_k w_k, oa (the count, with the fp32 rule of oa_pred), loss = sum_cw /
    sum_w, dlogits [n,2] = grad w_k / W (softmax_kc (t0 + t1) - t_kc), and the magnitudes the bounds are stated in:
        mu_k       = |t0 log t0| + |t1 log t1| + |t0| (|l0 - m| + |lg|) + |t1| (|l1 - m| + |lg|)       (the terms of cell_k; w = the weights)
        grad_mag_kc = |grad| w_k / W (softmax_kc |t0 + t1| + |t_kc|)
    grad_tiny_k = 2^-126 (1 + |grad| w_k / W |t0 + t1|) is what fp32 loses to underflow whatever the kernel: a softmax value below 2^-126 (logits
    more than 87 apart) is a subnormal float or 0, and so may be the product.  Against a target of exactly 0 the magnitude is that softmax value
    itself (1e-50 at a difference of 115), and no fp32 result is within a relative bound of it; the allowance is absolute and 1e-38."""
    l, t, w = logits.double(), gt[:, :2].double(), weights64(vol, norm)
    m = l.max(dim=1, keepdim=True).values
    a = l - m
    lg = torch.log1p(torch.exp(a.sum(dim=1, keepdim=True)))              # log(sum exp(x - max)) = log(1 + exp(-|l0 - l1|)), to the last bit when it is tiny
    tlogt = torch.where(t > 0, t * torch.log(t.clamp_min(1e-300)), torch.zeros_like(t))
    cell = (tlogt - t * (a - lg)).sum(dim=1)
    mu = (tlogt.abs() + t.abs() * (a.abs() + lg.abs())).sum(dim=1)
    sum_cw, sum_w = (cell * w).sum(), w.sum()
    pred = oa_pred(logits).to(t.device)
    oa = int(((t[:, 0] > t[:, 1]).long() == pred).sum())
    sm = torch.exp(a - lg)
    tt = t.sum(dim=1, keepdim=True)
    s = (float(grad) * w / sum_w)[:, None]
    return KL(sum_cw, sum_w, oa, sum_cw / sum_w, s * (sm * tt - t), mu, w, s.abs() * (sm * tt.abs() + t.abs()), TINY * (1 + s.abs() * tt.abs()), cell)


def chain(logits, gt, vol, norm, grad=1.0):
    """the reference's own op chain (learning/runModel.py:171-211) with torch ops in the dtype of `logits` -> (sum_cw, sum_w, loss, dlogits)"""
    lg = logits.detach().clone().requires_grad_(True)
    cell = F.kl_div(F.log_softmax(lg, dim=-1), gt[:, :2], reduction="none").sum(dim=1)
    w = torch.log(1 + vol) if norm == 1 else (torch.sqrt(vol) if norm == 2 else vol)
    cw = cell * w
    loss = cw.sum() / w.sum()
    (loss * grad).backward()
    return cw.sum().detach(), w.sum(), loss.detach(), lg.grad


LOSS_FLOOR = 2.0 ** -23


def kernel_rows(logits, gt, vol, norm):
    """(cell_k w_k, w_k) per row as loss.hip builds them (add_row): log t, log(sum exp(x - max)) and the weight each evaluated in fp64 and
    rounded once to fp32, combined in fp64"""
    f = lambda x: x.float().double()
    l, t = logits.double(), gt[:, :2].double()
    a = l - l.max(dim=1, keepdim=True).values
    lg = f(torch.log1p(torch.exp(a.sum(dim=1, keepdim=True))))
    tlogt = torch.where(t > 0, t * f(torch.log(t.clamp_min(1e-300))), torch.zeros_like(t))
    w = f(weights64(vol, norm))                                     # sqrtf is correctly rounded on the device; vol itself is an fp32 value
    return (tlogt - t * (a - lg)).sum(dim=1) * w, w


def grad_error(got, ref):
    """the worst element of |got - dlogits| beyond the underflow allowance, in units of grad_mag"""
    err = ((got.double() - ref.dlogits.to(got.device)).abs() - ref.grad_tiny.to(got.device)).clamp_min(0)
    mag = ref.grad_mag.to(got.device)
    return (err / mag.clamp_min(1e-300)).max().item()


def loss_bounds(logits, gt, vol, norm, grad, ref):
    """(B_sum, B_grad, e_sum, e_grad): the error of the reference's fp32 op chain, run with torch on the CPU on the same rows, in units of sum_k mu_k
    w_k (the weighted sum) and of grad_mag (the gradient, worst element, `grad_error`); B = max(4 e, 2^-23) as gemm_model.wgrad_bound -- the same terms in
    another order and with another libm"""
    c = lambda x: x.detach().float().cpu()
    s32, _, _, g32 = chain(c(logits), c(gt), c(vol), norm, grad)
    e_sum = (abs(s32.double() - ref.sum_cw.cpu()) / (ref.mu * ref.w).sum().cpu()).item()
    e_grad = grad_error(g32, ref)
    return max(4 * e_sum, LOSS_FLOOR), max(4 * e_grad, LOSS_FLOOR), e_sum, e_grad


# ---- loss: inputs -------------------------------------------------------------------------------------------------------------------------------------
def saturated_rows(n, gen):
    """(logits [n,2], gt [n,2], vol [n]) of the exact family: about half of the rows miss their target (cell term d), the rest hit it (0)"""
    d = torch.randint(128, 513, (n,), generator=gen).float()
    base = torch.randint(-3, 4, (n,), generator=gen).float()
    up = torch.randint(0, 2, (n,), generator=gen).bool()                 # class 1 has the larger logit
    logits = torch.stack([torch.where(up, base, base + d), torch.where(up, base + d, base)], 1)
    first = torch.randint(0, 2, (n,), generator=gen).float()             # target (1,0) or (0,1)
    return logits, torch.stack([first, 1 - first], 1), torch.randint(1, 8, (n,), generator=gen).float()


def saturated_sums(logits, gt, vol):
    """the three sums of saturated rows as integers, from the rows' definition (not through exp / log)"""
    d = (logits[:, 0] - logits[:, 1]).abs().double()
    miss = (gt[:, 0] > gt[:, 1]) == (logits[:, 1] > logits[:, 0])
    # the reference's counter compares [t0 > t1] (1 where the target is class 0) with the predicted index: it counts exactly the rows that miss
    return torch.stack([(d * miss * vol.double()).sum(), vol.double().sum(), miss.sum().double()])


def range_rows(n, kind, gen):
    """mixed: logits 3 randn; every fifth row a difference drawn from +-120; targets (p, 1 - p) with exact 0 and 1 among them; every third row's
    target scaled by a factor in [0.5, 2] (t0 + t1 != 1); one contiguous quarter of the rows well fitted, logits = log t + c, placed across the
    first block boundaries; vol = 10^U(-3, 3).  fitted: every row well fitted with normalised targets -- the loss cancels to about 0"""
    k = torch.arange(n)
    p = torch.rand(n, generator=gen) * 0.98 + 0.01
    c = torch.randn(n, generator=gen) * 3
    vol = torch.pow(10.0, torch.rand(n, generator=gen) * 6 - 3)
    fitted = torch.stack([torch.log(p) + c, torch.log1p(-p) + c], 1)
    if kind == "fitted":
        return fitted, torch.stack([p, 1 - p], 1), vol
    logits = 3 * torch.randn(n, 2, generator=gen)
    far = k % 5 == 1
    logits[:, 1] = torch.where(far, logits[:, 0] + (torch.rand(n, generator=gen) * 240 - 120), logits[:, 1])
    in_block = (k >= n // 3) & (k < n // 3 + n // 4)
    logits = torch.where(in_block[:, None], fitted, logits)
    p = torch.where((k % 7 == 0) & ~in_block, torch.zeros(n), p)
    p = torch.where((k % 11 == 3) & ~in_block, torch.ones(n), p)
    gt = torch.stack([p, 1 - p], 1) * torch.where(k % 3 == 2, torch.rand(n, generator=gen) * 1.5 + 0.5, torch.ones(n))[:, None]
    return logits, gt, vol


# rows at and below the resolution of the fp32 log-softmax: l1 - l0, and the mirrored differences
OA_DIFFS = (0.0, 1e-10, 1e-8, 1.2e-7, -1e-10, -1e-8, -1.2e-7)
OA_TARGETS = ((0.7, 0.3), (0.3, 0.7), (0.5, 0.5))


def oa_edge_rows():
    """(logits [21,2], gt [21,2]): every difference of OA_DIFFS on both sides of t0 > t1 and on t0 == t1.  Below half an ulp of log 2 (3e-8) the
    two log-softmax values are the same float and the reference counts class 0 whichever logit is larger"""
    L, T = [], []
    for d in OA_DIFFS:
        for t in OA_TARGETS:
            L.append((1e-10, 1e-10 + d) if d >= 0 else (1e-10 - d, 1e-10))
            T.append(t)
    return torch.tensor(L, dtype=torch.float32), torch.tensor(T, dtype=torch.float32)


def with_oa_rows(logits, gt, where):
    """copies of (logits, gt) with the rows of oa_edge_rows written from row `where` on"""
    L, T = oa_edge_rows()
    logits, gt = logits.clone(), gt.clone()
    logits[where:where + L.size(0)], gt[where:where + L.size(0), :2] = L, T
    return logits, gt
