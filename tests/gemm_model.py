"""CPU-side model of the dense-layer GEMM family (dgnn_amd/csrc/gemm.hip) for tests/test_gemm_model_cpu.py and tests/test_gpu_gemm_edges.py:
operands that sit inside larger buffers, inputs whose products are exact in every summation order, inputs with a wide dynamic range, fp64
references with their magnitudes, a mirror of the host dispatch and one table of cases per kernel variant.  No GPU import.

Exactness.  `ints` draws from {-3,-2,-1,1,2,3}: exact in bf16 and fp16 (and, times a power-of-two row scale, in the fp16 two-part form), never
zero.  A sum of K products is an integer of at most 9 K < 2^24, so every partial sum in every order, every split into bf16 parts and every
fp32 accumulation is exact: a correct kernel returns the fp64 result bit for bit, and a dropped, doubled or foreign term (a NaN from outside
the operand) always changes it.  `three_part` values a + b 2^-8 + c 2^-16 have non-zero bf16 hi, mid and lo parts (18 significant bits);
against a single-part operand, K <= 32 terms stay below 2^24 units of 2^-16 and are exact again -- only if all three parts are multiplied in.
"""
from __future__ import annotations

import os
import re
from collections import namedtuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the enum of include/dgnn_hip.h (dgnn_debug_last_linear_variant), mirrored; test_gemm_model_cpu.py compares it with the header ----------
VARIANTS = dict(NONE=0, F32=1, X3=2, X3_N64=3, X3_BIG=4, X3_MID1=5, X3_MID4=6, X3_SMALL=7, X3_SMALL_SPLITK=8, B=9, B_MID1=10, B_MID4=11,
                B_SMALL=12, B_SMALL_SPLITK=13, X2H=14, X2HP=15)
VARIANT_NAMES = {v: k for k, v in VARIANTS.items()}


def header_variants():
    src = open(os.path.join(ROOT, "include", "dgnn_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\bDGNN_LINEAR_VARIANT_([A-Z0-9_]+)\s*=\s*(\d+)", src)}


# ---- operands inside larger buffers -----------------------------------------------------------------------------------------------------
def embed(t, pad_rows=2, pad_cols_before=3, pad_cols_after=2, fill=float("nan"), misalign=0, stride_mult4=None):
    """A view with t's values (t: [rows, cols], on t's device) inside a larger buffer filled with `fill`: `pad_rows` rows after the last,
    `pad_cols_before` / `pad_cols_after` columns on both sides of every row.  `misalign`: bytes (0, 4, 8, 12; a multiple of the element size)
    by which the view's first element is off 16-byte alignment.  `stride_mult4`: True makes the row stride a multiple of 16 bytes (4 fp32 or 8
    bf16 elements: the kernels' vector loads are allowed when the base is aligned too), False makes it no multiple of 4 elements, None leaves
    pad_cols_before + cols + pad_cols_after.  The buffer is `view._base`; see `outside_intact`."""
    rows, cols = t.shape
    es = t.element_size()
    assert misalign % es == 0 and 0 <= misalign < 16
    ld = pad_cols_before + cols + pad_cols_after
    if stride_mult4 is True:
        q = 16 // es
        ld = (ld + q - 1) // q * q
    elif stride_mult4 is False and ld % 4 == 0:
        ld += 1
    q = 16 // es
    off = (-pad_cols_before) % q + misalign // es + q          # first element of the view: 16-byte aligned + misalign, with q fill elements in front
    buf = torch.full((off + (rows + pad_rows) * ld + q,), fill, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = torch.as_strided(buf, (rows, cols), (ld, 1), off + pad_cols_before)
    view.copy_(t)
    assert view.data_ptr() % 16 == misalign and view._base is buf
    return view


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def outside_intact(view, fill):
    """True if every element of view's buffer that is not part of the view still holds `fill` (bit pattern; fill may be NaN)."""
    buf = view._base
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    torch.as_strided(keep, view.shape, view.stride(), view.storage_offset()).fill_(False)
    want = _bits(torch.full((1,), fill, dtype=buf.dtype, device=buf.device))
    return bool((_bits(buf)[keep] == want).all())


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
_SET = torch.tensor([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0])


def ints(shape, gen):
    """fp32 values from {-3,-2,-1,1,2,3}"""
    return _SET[torch.randint(0, 6, tuple(shape), generator=gen)]


def three_part(shape, gen):
    """a + b 2^-8 + c 2^-16 with a, b, c from `ints`: 18 significant bits.  The kernels split by rounding to nearest (fused_common.h split3), and
    for some draws that leaves a part empty (2^-8 + 2 * 2^-16 has 8 bits; with a = +-1 the residual after the hi part always fits the mid part):
    those entries are drawn again until the hi, mid and lo parts are all non-zero."""
    a, b, c = ints(shape, gen), ints(shape, gen), ints(shape, gen)
    for _ in range(200):
        v = a + b * 2.0 ** -8 + c * 2.0 ** -16
        hi = bf16_round(v)
        mid = bf16_round(v - hi)
        bad = (mid == 0) | (v - hi - mid == 0)
        if not bad.any():
            return v
        a, b, c = (torch.where(bad, ints(shape, gen), t) for t in (a, b, c))
    raise AssertionError("three_part: no draw with three non-zero parts")


def pow2(shape, gen, lo=-3, hi=3):
    """+-2^e with one exponent e in [lo, hi] per row and a sign per element: a single-part operand.  One exponent per row scales a whole dot
    product, so the exactness of sums of `ints` and `three_part` terms carries over"""
    e = torch.randint(lo, hi + 1, (shape[0],) + (1,) * (len(shape) - 1), generator=gen).float()
    return torch.exp2(e) * (torch.randint(0, 2, tuple(shape), generator=gen).float() * 2 - 1)


def wide(shape, gen, row_exp=(0, 0)):
    """randn * 2^U{-6..6} per element, times 2^e per row; e drawn from U{row_exp[0]..row_exp[1]}, the first rows taking both ends"""
    rows = shape[0]
    e = torch.randint(row_exp[0], row_exp[1] + 1, (rows, 1), generator=gen)
    e[0, 0] = row_exp[1]
    e[-1, 0] = row_exp[0]
    el = torch.randint(-6, 7, tuple(shape), generator=gen)
    return torch.randn(tuple(shape), generator=gen) * torch.exp2((el + e).float())


def bf16_round(t):
    return t.to(torch.bfloat16).float()


# ---- fp64 references ------------------------------------------------------------------------------------------------------------------------
def ref_fwd(A1, W1, A2=None, W2=None, bias=None, scale=None, shift=None, relu=False):
    """(act((A1 W1^T + A2 W2^T + bias) * scale + shift), (|A1||W1|^T + |A2||W2|^T + |bias|) * |scale| + |shift|) in fp64, on the operands' device"""
    d = lambda t: t.double()
    r = d(A1) @ d(W1).t()
    m = d(A1).abs() @ d(W1).abs().t()
    if A2 is not None:
        r = r + d(A2) @ d(W2).t()
        m = m + d(A2).abs() @ d(W2).abs().t()
    if bias is not None:
        r, m = r + d(bias), m + d(bias).abs()
    if scale is not None:
        r, m = r * d(scale) + d(shift), m * d(scale).abs() + d(shift).abs()
    if relu:
        r = r.clamp_min(0)
    return r, m


def ref_wgrad(A, B):
    """(A^T B, |A|^T |B|) in fp64"""
    a, b = A.double(), B.double()
    return a.t() @ b, a.abs().t() @ b.abs()


def ref_colsum(A):
    a = A.double()
    return a.sum(0), a.abs().sum(0)


def seq_sum_fp32(A, W):
    """A W^T as a plain fp32 sequential sum over k (rounded product, rounded add): the longest chain an fp32 kernel could run"""
    acc = torch.zeros(A.size(0), W.size(0), dtype=torch.float32)
    for k in range(A.size(1)):
        acc = acc + A[:, k:k + 1] * W[:, k][None, :]
    return acc


# The per-element bounds of the range tests, in units of the magnitude.  Forward: the project's own constants (test_small_gemm_split_k_form).
C_FWD_F32 = 2e-6      # f32, x3, x2h / x2hp
C_FWD_BF16 = 4e-6     # bf16 storage, against the operands as rounded
WGRAD_FLOOR = 2.0 ** -23


def wgrad_bound(cpu_err):
    """four times the error of a plain fp32 CPU matmul on the same inputs (in units of |A|^T|B|), and not less than 2^-23: both are fp32 sums
    of the same terms in different orders, and the kernel's order (row splits, then a two-level reduce) is the shorter chain"""
    return max(4.0 * cpu_err, WGRAD_FLOOR)


# ---- the host dispatch, mirrored (linear_fwd_x3_impl / dgnn_linear_fwd_bf16 in gemm.hip) ---------------------------------------------------
NUM_CU = 256
SWITCHES = ("DGNN_X3_BIG", "DGNN_X3_SMALL", "DGNN_X3_N64", "DGNN_BF16_SMALL", "DGNN_SMALL_BY_TILES", "DGNN_GEMM_MID", "DGNN_GEMM_MID_KS",
            "DGNN_SMALL_SPLITK")


def env_switches(env=None):
    env = os.environ if env is None else env
    return {s: not env.get(s, "1").startswith("0") for s in SWITCHES}


def _cdiv(a, b):
    return -(-a // b)


def x3_variant(M, n_out, K, on=None):
    on = on or {s: True for s in SWITCHES}
    tiles = lambda tm, tn: _cdiv(M, tm) * _cdiv(n_out, tn)
    tiles_fill = on["DGNN_SMALL_BY_TILES"] and K >= 128 and n_out > 64 and tiles(128, 128) >= 150
    if on["DGNN_X3_BIG"] and M >= 8192 and n_out > 128 and tiles(256, 256) >= 192:
        return "X3_BIG"
    if on["DGNN_GEMM_MID"] and not tiles_fill and M <= 16384 and n_out > 64 and K >= 512 and tiles(64, 64) >= 128:
        return "X3_MID4" if on["DGNN_GEMM_MID_KS"] and K >= 1024 and tiles(64, 64) <= 2 * NUM_CU else "X3_MID1"
    if on["DGNN_X3_SMALL"] and not tiles_fill and M <= 16384:
        return "X3_SMALL_SPLITK" if on["DGNN_SMALL_SPLITK"] and K >= 1024 else "X3_SMALL"
    if on["DGNN_X3_N64"] and n_out <= 64:
        return "X3_N64"
    return "X3"


def bf16_variant(M, n_out, K, on=None):
    on = on or {s: True for s in SWITCHES}
    tiles = lambda tm, tn: _cdiv(M, tm) * _cdiv(n_out, tn)
    tiles_fill = on["DGNN_SMALL_BY_TILES"] and K >= 128 and tiles(128, 64) >= 150
    if on["DGNN_GEMM_MID"] and not tiles_fill and M <= 16384 and K >= 512 and tiles(64, 64) >= 128:
        return "B_MID4" if on["DGNN_GEMM_MID_KS"] and K >= 1024 and tiles(64, 64) <= 2 * NUM_CU else "B_MID1"
    if on["DGNN_BF16_SMALL"] and not tiles_fill and on["DGNN_SMALL_SPLITK"] and M <= 16384 and K >= 1024:
        return "B_SMALL_SPLITK"
    if on["DGNN_BF16_SMALL"] and not tiles_fill and M <= 16384:
        return "B_SMALL"
    return "B"


def expected_variant(entry, M, n_out, K, on=None):
    """entry: f32 | x3 | bf16 | x2h | x2hp (the C entry point); None where x2h / x2hp return DGNN_E_UNSUPPORTED"""
    if entry == "f32":
        return "F32"
    if entry in ("x2h", "x2hp"):
        return entry.upper() if M >= 8192 and n_out > 128 else None
    return x3_variant(M, n_out, K, on) if entry == "x3" else bf16_variant(M, n_out, K, on)


def wgrad_plan(M, n_a, chunk):
    """(splits, rows_per_split, rows in the last split that has any) of a weight gradient; chunk: 32 (f32, x3) or 64 (bf16 kernels)"""
    s = _cdiv(M, 128)
    cap = max(512 // _cdiv(n_a, 64), 32)
    splits = max(1, min(s, cap))
    rps = max(_cdiv(_cdiv(M, splits), chunk) * chunk, chunk)
    last = M - (_cdiv(M, rps) - 1) * rps
    return splits, rps, last


# ---- the case table ---------------------------------------------------------------------------------------------------------------------------
# One canonical row per variant -- the smallest shape that reaches it under the default switches, from the dispatch conditions above -- then the
# ragged rows: last row block of 1 row and of tile-1 rows, n_out one past and one short of the tile width, k1 and k2 no multiples of 32 or 4 (the
# [A1|A2] seam inside a chunk), k2 = 0.  `switch`: the environment switches that, set to 0, take the variant away.
Case = namedtuple("Case", "variant entry M n_out k1 k2 switch")


def _rows(variant, entry, switch, shapes):
    return [Case(variant, entry, M, n, k1, k2, switch) for (M, n, k1, k2) in shapes]


_SMALL = [(33, 33, 3, 2), (63, 31, 31, 0), (1, 1, 1, 0), (97, 65, 37, 30), (32, 32, 32, 32)]                  # 32 x 32 blocks, 4 per workgroup
_SPLITK = [(33, 33, 1030, 77), (63, 31, 1025, 0), (1, 64, 1024, 0)]                                          # K >= 1024, n_out <= 64 keeps mid away
_MID1 = [(1000, 512, 512, 0), (961, 449, 301, 215), (1023, 511, 513, 0)]                                     # 16 x 8 = 128 tiles of 64, 512 <= K < 1024
_MID4 = [(1000, 512, 1024, 0), (961, 449, 613, 415), (1023, 511, 1025, 0)]                                   # K >= 1024, tiles64 <= 512
_T128 = [(16384 + 1 + 77, 65, 3, 2), (129 * 128 + 1, 129, 37, 30), (129 * 128 + 127, 127, 33, 0)]            # M > 16384: 128-row tiles
_WIDE = [(8193, 129, 3, 2), (8192 + 255, 257, 37, 30), (8192 + 77, 255, 33, 0)]                              # x2h / x2hp: M >= 8192, n_out > 128

CASES = (
    _rows("F32", "f32", (), [(129, 65, 3, 2), (255, 63, 37, 30), (1, 1, 1, 0), (128, 64, 33, 0)])
    + _rows("X3_SMALL", "x3", ("DGNN_X3_SMALL",), _SMALL)
    + _rows("X3_SMALL_SPLITK", "x3", ("DGNN_X3_SMALL", "DGNN_SMALL_SPLITK"), _SPLITK)
    + _rows("X3_MID1", "x3", ("DGNN_GEMM_MID",), _MID1)
    + _rows("X3_MID4", "x3", ("DGNN_GEMM_MID", "DGNN_GEMM_MID_KS"), _MID4)
    + _rows("X3", "x3", (), _T128 + [(75 * 128 + 1, 129, 100, 29)])                      # the last: M <= 16384, kept off the small kernels by 150 tiles
    + _rows("X3_N64", "x3", ("DGNN_X3_N64",), [(16384 + 1 + 77, 64, 3, 2), (129 * 128 + 1, 63, 37, 30), (129 * 128 + 127, 1, 33, 0)])
    # 256 x 256 tiles, at least 192 of them: 33 x 6.  A last row block of 255 rows would need 8447 x 1281 outputs, more than the suite's largest
    # (8269 x 1300); the 77-row block stands in for it
    + _rows("X3_BIG", "x3", ("DGNN_X3_BIG",), [(8192 + 77, 1300, 5, 3), (8193, 1281, 37, 0)])
    + _rows("X2H", "x2h", (), _WIDE)
    + _rows("X2HP", "x2hp", (), _WIDE)
    + _rows("B_SMALL", "bf16", ("DGNN_BF16_SMALL",), _SMALL)
    + _rows("B_SMALL_SPLITK", "bf16", ("DGNN_BF16_SMALL", "DGNN_SMALL_SPLITK"), _SPLITK)
    + _rows("B_MID1", "bf16", ("DGNN_GEMM_MID",), _MID1)
    + _rows("B_MID4", "bf16", ("DGNN_GEMM_MID", "DGNN_GEMM_MID_KS"), _MID4)
    + _rows("B", "bf16", (), [(16384 + 1 + 77, 65, 3, 2), (129 * 128 + 1, 63, 67, 62), (129 * 128 + 127, 64, 65, 0), (19 * 128 + 1, 449, 100, 29)])
)


def case_id(c):
    return "%s-%dx%d-k%d+%d" % (c.variant, c.M, c.n_out, c.k1, c.k2)


# wide-range cases: one per variant (the canonical row, K raised where the variant allows, so that the sums are long)
RANGE_CASES = [
    Case("F32", "f32", 300, 70, 2048, 77, ()),
    Case("X3_SMALL", "x3", 97, 65, 300, 211, ("DGNN_X3_SMALL",)),
    Case("X3_SMALL_SPLITK", "x3", 63, 33, 2048, 77, ("DGNN_X3_SMALL", "DGNN_SMALL_SPLITK")),
    Case("X3_MID1", "x3", 961, 449, 700, 215, ("DGNN_GEMM_MID",)),
    Case("X3_MID4", "x3", 961, 449, 2048, 77, ("DGNN_GEMM_MID", "DGNN_GEMM_MID_KS")),
    Case("X3", "x3", 75 * 128 + 1, 129, 300, 211, ()),
    Case("X3_N64", "x3", 16384 + 78, 63, 300, 211, ("DGNN_X3_N64",)),
    Case("X3_BIG", "x3", 8192 + 77, 1300, 100, 29, ("DGNN_X3_BIG",)),
    Case("X2H", "x2h", 8193, 257, 300, 211, ()),
    Case("X2HP", "x2hp", 8193, 257, 300, 211, ()),
    Case("B_SMALL", "bf16", 97, 65, 300, 211, ("DGNN_BF16_SMALL",)),
    Case("B_SMALL_SPLITK", "bf16", 63, 33, 2048, 77, ("DGNN_BF16_SMALL", "DGNN_SMALL_SPLITK")),
    Case("B_MID1", "bf16", 961, 449, 700, 215, ("DGNN_GEMM_MID",)),
    Case("B_MID4", "bf16", 961, 449, 2048, 77, ("DGNN_GEMM_MID", "DGNN_GEMM_MID_KS")),
    Case("B", "bf16", 19 * 128 + 1, 449, 300, 211, ()),
]
# row exponents of the range tests: (A rows, W rows).  A at 2^+60 against W at 2^-60 and the reverse keep every product inside fp32's range
ROW_EXPS = {"mid": ((-8, 8), (-8, 8)), "a_big": ((50, 60), (-60, -50)), "w_big": ((-60, -50), (50, 60))}

# weight gradients
WGRAD_M = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
WGRAD_N = ((1, 130), (63, 65), (64, 64), (65, 63), (130, 1))           # (n_a, n_b): every width of {1, 63, 64, 65, 130} on both sides
# the capped regime: n_a >= 1024 caps the splits at 32.  M = 4100: 32 splits of 160 rows, 26..31 empty (f32 / x3, 32-row chunks).  The bf16
# kernels round the split to 64-row chunks (192 rows here): M = 22 * 192 + 1 leaves one row for split 22 and nothing for 23..31.
WGRAD_CAPPED = ((4100, 1024, 3), (4100, 1025, 3), (22 * 192 + 1, 1024, 3))
