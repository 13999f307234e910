"""Every dense-layer GEMM variant of dgnn_amd/csrc/gemm.hip at its edges (tests/gemm_model.py has the cases, the inputs and the arguments):
exact results on integer inputs with every operand inside a NaN-filled buffer and every output inside a canary buffer, the three bf16 parts of
the x3 split, per-element fp64 bounds on inputs with a wide dynamic range, and locality of a NaN / Inf.  Each forward case asserts the kernel
it reached (dgnn_debug_last_linear_variant).  Raw library calls: ops hides ldo, lddw and accumulate."""
import functools
import os

import pytest
import torch

import gemm_model as gm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CANARY = -(2.0 ** 20)          # exact in fp32 and bf16, larger than any exact result here


def _lib():
    from dgnn_amd._lib import check, lib, ptr, stream_ptr
    return lib(), ptr, stream_ptr, check


def _ld(t):
    return 0 if t is None else t.stride(0)


def fwd_raw(entry, A1, W1, A2, W2, bias, scale, shift, relu, out):
    """one forward call through the C entry point `entry` names; -> the variant it reached"""
    lib, ptr, stream_ptr, check = _lib()
    M, k1 = A1.shape
    n_out = W1.size(0)
    k2 = A2.size(1) if A2 is not None else 0
    assert W1.size(1) == k1 and out.shape == (M, n_out) and (A2 is None or (A2.size(0) == M and W2.shape == (n_out, k2)))
    assert all(t is None or t.stride(1) == 1 for t in (A1, W1, A2, W2, out)) and all(t is None or t.numel() == n_out for t in (bias, scale, shift))
    args = (ptr(A1), _ld(A1), k1, ptr(W1), _ld(W1), ptr(A2), _ld(A2), k2, ptr(W2), _ld(W2), ptr(bias), ptr(scale), ptr(shift), int(relu), M, n_out,
            ptr(out), _ld(out))
    if entry == "bf16":
        assert A1.dtype == torch.bfloat16 and W1.dtype == torch.float32
        check(lib.dgnn_linear_fwd_bf16(*args, int(out.dtype == torch.float32), stream_ptr()), "dgnn_linear_fwd_bf16")
    elif entry in ("x2h", "x2hp"):
        n = lib.dgnn_linear_fwd_x2h_scratch_elems(M, n_out) if entry == "x2h" else lib.dgnn_linear_fwd_x2hp_scratch_elems(M, n_out, k1, k2)
        scratch = torch.full((int(n),), NAN, dtype=torch.float32, device=DEV)
        check(getattr(lib, "dgnn_linear_fwd_" + entry)(*args, scratch.data_ptr(), stream_ptr()), entry)
    else:
        check((lib.dgnn_linear_fwd if entry == "f32" else lib.dgnn_linear_fwd_x3)(*args, stream_ptr()), entry)
    torch.cuda.synchronize()
    return gm.VARIANT_NAMES[lib.dgnn_debug_last_linear_variant()]


def assert_variant(c, got):
    off = [s for s in c.switch if os.environ.get(s, "1").startswith("0")]
    if off:
        pytest.skip("%s is off: %s=0" % (c.variant, off[0]))
    assert got == c.variant, "%s reached %s" % (gm.case_id(c), got)


def place(t, mode, which=0, dtype=None):
    """an operand on the device inside a NaN-filled buffer.  mode vec: base and stride allow 16-byte loads; scalar: operand 0 of a pair sits 4, 8
    or 12 bytes off with a stride that would allow them, operand 1 on an aligned base with a stride that is no multiple of 4 elements"""
    if t is None:
        return None
    t = t.to(DEV)
    if dtype is not None:
        t = t.to(dtype)
    if mode == "vec":
        return gm.embed(t, 2, 3, 2, NAN, 0, True)
    if which % 2 == 0:
        return gm.embed(t, 2, 3, 2, NAN, (4, 8, 12)[(t.size(0) + which // 2) % 3], True)
    return gm.embed(t, 2, 3, 2, NAN, 0, False)


def out_buffer(M, n_out, dtype=torch.float32, init=None):
    """the output inside a canary buffer: ldo = n_out + 3, two extra rows"""
    t = torch.full((M, n_out), NAN, dtype=dtype, device=DEV) if init is None else init.to(DEV).to(dtype)
    return gm.embed(t, 2, 0, 3, CANARY)


@functools.lru_cache(maxsize=None)
def exact_case(c):
    """integer operands of a table row and the fp64 result before the ReLU, computed once per row"""
    gen = torch.Generator().manual_seed(c.M + 3 * c.n_out + 5 * c.k1 + c.k2)
    A1, W1 = gm.ints((c.M, c.k1), gen), gm.ints((c.n_out, c.k1), gen)
    A2, W2 = (gm.ints((c.M, c.k2), gen), gm.ints((c.n_out, c.k2), gen)) if c.k2 else (None, None)
    bias, shift, scale = gm.ints((c.n_out,), gen).to(DEV), gm.ints((c.n_out,), gen).to(DEV), gm.pow2((c.n_out,), gen).to(DEV)
    dev = lambda t: None if t is None else t.to(DEV)
    ref, mag = gm.ref_fwd(dev(A1), dev(W1), dev(A2), dev(W2), bias, scale, shift)
    assert mag.max().item() < 2.0 ** 24
    return (A1, W1, A2, W2), (bias, scale, shift), ref


def _out_types(c):
    return (torch.float32, torch.bfloat16) if c.entry == "bf16" else (torch.float32,)


@pytest.mark.parametrize("mode", ["vec", "scalar"])
@pytest.mark.parametrize("c", gm.CASES, ids=gm.case_id)
def test_forward_exact_on_every_variant(c, mode):
    """Integer operands, integer bias and shift, power-of-two scale: the result is exact in every order, so `out` equals the fp64 reference
    (rounded once to bf16 for bf16 output), with ReLU and without, the canary around `out` (ldo = n_out + 3, two rows below) is intact, and no
    NaN from the buffers around the operands got in.  The variant reached is the one the table names.
    x2h / x2hp: the row scales are powers of two (x2h_scale_of builds them from the exponent of the row maximum) and 3 * 2^13 is an fp16 value,
    so the two-part form is exact on these inputs as well and takes the same assertions."""
    ops_, (bias, scale, shift), ref = exact_case(c)
    adt = torch.bfloat16 if c.entry == "bf16" else None
    A1, A2 = place(ops_[0], mode, 0, adt), place(ops_[2], mode, 1, adt)
    W1, W2 = place(ops_[1], mode, 2), place(ops_[3], mode, 3)
    for odt in _out_types(c):
        for relu in (1, 0):
            out = out_buffer(c.M, c.n_out, odt)
            got = fwd_raw(c.entry, A1, W1, A2, W2, bias, scale, shift, relu, out)
            assert_variant(c, got)
            want = ref.clamp_min(0) if relu else ref
            assert not torch.isnan(out).any(), "NaN in out"
            assert torch.equal(out.double(), want.to(odt).double()), "out differs: max %g" % (out.double() - want).abs().max().item()
            assert gm.outside_intact(out, CANARY), "canary moved"
    for t in (A1, W1, A2, W2):
        assert t is None or gm.outside_intact(t, NAN)


def test_forward_plain_call_without_epilogue_and_accumulate_flag():
    """no bias, no scale / shift, and DGNN_LINEAR_ACCUMULATE onto integer contents (f32 and x3 kernels), ldo > n_out"""
    c = gm.Case("X3_SMALL", "x3", 97, 65, 37, 30, ("DGNN_X3_SMALL",))
    (A1, W1, A2, W2), _, _ = exact_case(c)
    ref, _ = gm.ref_fwd(A1, W1, A2, W2)
    init = gm.ints((c.M, c.n_out), torch.Generator().manual_seed(1))
    a1, w1, a2, w2 = place(A1, "scalar", 0), place(W1, "scalar", 2), place(A2, "scalar", 1), place(W2, "scalar", 3)
    for entry in ("f32", "x3"):
        out = out_buffer(c.M, c.n_out)
        fwd_raw(entry, a1, w1, a2, w2, None, None, None, 0, out)
        assert torch.equal(out.double().cpu(), ref) and gm.outside_intact(out, CANARY)
        out = out_buffer(c.M, c.n_out, init=init)
        fwd_raw(entry, a1, w1, a2, w2, None, None, None, 2, out)
        assert torch.equal(out.double().cpu(), ref + init.double()) and gm.outside_intact(out, CANARY)


def test_ops_linear_fwd_reaches_the_mode_s_entry_point(monkeypatch):
    """ops.linear_fwd under the three GEMM modes it distinguishes: f32 -> k_linear_fwd, bf16x3 -> the x3 family, f16x2 -> the fp16 two-part
    form for M >= 8192 and n_out > 256 (and the x3 family below)"""
    from dgnn_amd import ops
    lib = _lib()[0]
    gen = torch.Generator().manual_seed(3)
    M, n_out, k = 8193, 257, 37
    A, W = gm.ints((M, k), gen).to(DEV), gm.ints((n_out, k), gen).to(DEV)
    ref, _ = gm.ref_fwd(A, W)
    last = lambda: gm.VARIANT_NAMES[lib.dgnn_debug_last_linear_variant()]
    for mode, want, want_small in ((ops.GEMM_F32, "F32", "F32"), (ops.GEMM_BF16X3, gm.x3_variant(M, n_out, k, gm.env_switches()), gm.x3_variant(97, n_out, k, gm.env_switches())),
                                   (ops.GEMM_F16X2, "X2HP" if ops.X2HP else "X2H", gm.x3_variant(97, n_out, k, gm.env_switches()))):
        monkeypatch.setattr(ops, "GEMM_MODE", mode)
        assert torch.equal(ops.linear_fwd(A, W).double(), ref) and last() == want
        assert torch.equal(ops.linear_fwd(A[:97], W).double(), ref[:97]) and last() == want_small


THREE_PART_SHAPES = [gm.Case("X3_SMALL", "x3", 70, 33, 0, 0, ("DGNN_X3_SMALL",)), gm.Case("X3", "x3", 16384 + 78, 65, 0, 0, ()),
                     gm.Case("X3_N64", "x3", 16384 + 78, 33, 0, 0, ("DGNN_X3_N64",)), gm.Case("X3_BIG", "x3", 8193, 1281, 0, 0, ("DGNN_X3_BIG",))]


@pytest.mark.parametrize("K", [1, 31, 32])
@pytest.mark.parametrize("c", THREE_PART_SHAPES, ids=lambda c: c.variant)
def test_forward_three_parts_exact(c, K):
    """18-bit operands whose bf16 hi, mid and lo parts are all non-zero against single-part powers of two, then the other way round: at most 32
    terms are exact in fp32, so the x3 kernels return the fp64 result only if every part of either operand is multiplied in."""
    gen = torch.Generator().manual_seed(K + c.n_out)
    for a_three in (True, False):
        A = (gm.three_part if a_three else gm.pow2)((c.M, K), gen)
        W = (gm.pow2 if a_three else gm.three_part)((c.n_out, K), gen)
        a, w = place(A, "scalar", 0), place(W, "vec", 2)
        out = out_buffer(c.M, c.n_out)
        assert_variant(c, fwd_raw("x3", a, w, None, None, None, None, None, 0, out))
        ref, _ = gm.ref_fwd(a, w)
        assert torch.equal(out.double(), ref) and gm.outside_intact(out, CANARY)


@pytest.mark.parametrize("exps", sorted(gm.ROW_EXPS))
@pytest.mark.parametrize("c", gm.RANGE_CASES, ids=gm.case_id)
def test_forward_range(c, exps):
    """randn * 2^U{-6..6} per element, rows of A at 2^+60 against rows of W at 2^-60 (and the reverse, and both within 2^+-8): every element
    within c * (|A||W|^T + |bias|) |scale| + |shift| of fp64, c = 2e-6 for the fp32-class kernels (f32, x3, x2h, x2hp) and 4e-6 for bf16 storage
    against the operands as rounded -- the constants of test_small_gemm_split_k_form.  Bias, BatchNorm scale / shift and ReLU on."""
    ea, ew = gm.ROW_EXPS[exps]
    gen = torch.Generator().manual_seed(c.M + c.k1 + len(exps))
    A1, W1 = gm.wide((c.M, c.k1), gen, ea), gm.wide((c.n_out, c.k1), gen, ew)
    A2, W2 = gm.wide((c.M, c.k2), gen, ea), gm.wide((c.n_out, c.k2), gen, ew)
    bias, scale, shift = (torch.randn(c.n_out, generator=gen).to(DEV), (torch.rand(c.n_out, generator=gen) + 0.5).to(DEV),
                          (torch.randn(c.n_out, generator=gen) * 0.1).to(DEV))
    bf = c.entry == "bf16"
    adt = torch.bfloat16 if bf else None
    a1, a2, w1, w2 = place(A1, "vec", 0, adt), place(A2, "scalar", 1, adt), place(W1, "vec", 2), place(W2, "scalar", 3)
    out = out_buffer(c.M, c.n_out)
    assert_variant(c, fwd_raw(c.entry, a1, w1, a2, w2, bias, scale, shift, 1, out))
    rnd = (lambda t: gm.bf16_round(t)) if bf else (lambda t: t)
    ref, mag = gm.ref_fwd(a1.float(), rnd(w1), a2.float(), rnd(w2), bias, scale, shift, relu=True)
    err = ((out.double() - ref).abs() / mag).max().item()
    print("range %s %s: %.3g of the magnitude" % (gm.case_id(c), exps, err))
    assert torch.isfinite(out).all() and gm.outside_intact(out, CANARY)
    assert err <= (gm.C_FWD_BF16 if bf else gm.C_FWD_F32)


# ---- weight gradients -------------------------------------------------------------------------------------------------------------------------------
WGRAD_KERNELS = ("f32", "x3", "b_ff", "b_fb", "b_bf", "b_bb")       # b_<A><B>: dgnn_linear_wgrad_bf16 with fp32 (f) or bf16 (b) storage per operand
CAT_KERNELS = ("x3_cat", "bcat_ff", "bcat_fb", "bcat_bf", "bcat_bb")


def _dt(ch):
    return torch.float32 if ch == "f" else torch.bfloat16


def wgrad_raw(kind, A, B, dW, accumulate):
    lib, ptr, stream_ptr, check = _lib()
    M, na = A.shape
    nb = B.size(1)
    assert B.size(0) == M and dW.shape == (na, nb)
    partials = torch.full((int(lib.dgnn_linear_wgrad_scratch_elems(M, na, nb)),), NAN, dtype=torch.float32, device=DEV)
    if kind in ("f32", "x3"):
        fn = lib.dgnn_linear_wgrad if kind == "f32" else lib.dgnn_linear_wgrad_x3
        check(fn(ptr(A), _ld(A), na, ptr(B), _ld(B), nb, M, ptr(dW), _ld(dW), accumulate, ptr(partials), stream_ptr()), kind)
    else:
        assert A.dtype == _dt(kind[2]) and B.dtype == _dt(kind[3])
        check(lib.dgnn_linear_wgrad_bf16(ptr(A), int(kind[2] == "f"), _ld(A), na, ptr(B), int(kind[3] == "f"), _ld(B), nb, M, ptr(dW), _ld(dW), accumulate,
                                         ptr(partials), stream_ptr()), kind)
    torch.cuda.synchronize()


def wgrad_cat_raw(kind, A, B1, B2, dW1, dW2, db):
    lib, ptr, stream_ptr, check = _lib()
    M, na = A.shape
    nb1, nb2 = B1.size(1), (B2.size(1) if B2 is not None else 0)
    assert dW1.is_contiguous() and dW1.shape == (na, nb1) and (B2 is None or (dW2.is_contiguous() and dW2.shape == (na, nb2))) and (db is None or db.numel() == na)
    scratch = torch.full((int(lib.dgnn_linear_wgrad_cat_scratch_elems(M, na, nb1, nb2)),), NAN, dtype=torch.float32, device=DEV)
    if kind == "x3_cat":
        check(lib.dgnn_linear_wgrad_x3_cat(ptr(A), _ld(A), na, ptr(B1), _ld(B1), nb1, ptr(B2), _ld(B2), nb2, M, ptr(dW1), ptr(dW2), ptr(db), ptr(scratch),
                                           stream_ptr()), kind)
    else:
        assert A.dtype == _dt(kind[5]) and B1.dtype == _dt(kind[6])
        check(lib.dgnn_linear_wgrad_bf16_cat(ptr(A), int(kind[5] == "f"), _ld(A), na, ptr(B1), _ld(B1), nb1, ptr(B2), _ld(B2), nb2, int(kind[6] == "f"), M,
                                             ptr(dW1), ptr(dW2), ptr(db), ptr(scratch), stream_ptr()), kind)
    torch.cuda.synchronize()


def _operand_types(kind):
    if kind in ("f32", "x3", "x3_cat"):
        return torch.float32, torch.float32
    return _dt(kind[-2]), _dt(kind[-1])


def check_wgrad_exact(kind, M, na, nb, mode, seed):
    gen = torch.Generator().manual_seed(seed)
    A, B, init = gm.ints((M, na), gen), gm.ints((M, nb), gen), gm.ints((na, nb), gen)
    ta, tb = _operand_types(kind)
    a, b = place(A, mode, 0, ta), place(B, mode, 1 if mode == "scalar" else 0, tb)
    ref, _ = gm.ref_wgrad(a, b)
    for acc in (0, 1):
        dW = gm.embed((init if acc else torch.full((na, nb), NAN)).to(DEV), 2, 0, 5, CANARY)
        assert dW.stride(0) == nb + 5
        wgrad_raw(kind, a, b, dW, acc)
        want = ref + init.double().to(DEV) if acc else ref
        where = "%s M=%d n_a=%d n_b=%d %s accumulate=%d" % (kind, M, na, nb, mode, acc)
        assert not torch.isnan(dW).any(), where
        assert torch.equal(dW.double(), want), where
        assert gm.outside_intact(dW, CANARY), where


@pytest.mark.parametrize("M", gm.WGRAD_M)
@pytest.mark.parametrize("kind", WGRAD_KERNELS)
def test_wgrad_exact(kind, M):
    """dW = A^T B on integer operands inside NaN-filled buffers (NaN rows after M, NaN columns on both sides), dW inside a canary buffer with
    lddw = n_b + 5, partials NaN-filled: equal to fp64 with accumulate = 0 (dW holds NaN before) and with accumulate = 1 onto integer contents.
    M at every edge of the 32- and 64-row chunks and of the 128-row split rule, widths {1, 63, 64, 65, 130} on both sides."""
    for i, (na, nb) in enumerate(gm.WGRAD_N):
        check_wgrad_exact(kind, M, na, nb, ("vec", "scalar")[(i + M) % 2], M * 7 + i)


@pytest.mark.parametrize("M,na,nb", gm.WGRAD_CAPPED)
@pytest.mark.parametrize("kind", WGRAD_KERNELS)
def test_wgrad_exact_where_the_splits_are_capped(kind, M, na, nb):
    """n_a >= 1024 caps the row splits at 32 and the rounding of rows_per_split leaves the trailing splits without rows: M = 4100 gives 32
    splits of 160 rows (f32, x3), 26..31 empty; M = 4225 gives the bf16 kernels (192 rows per split) a last split of one row."""
    chunk = 32 if kind in ("f32", "x3") else 64
    splits, rps, last = gm.wgrad_plan(M, na, chunk)
    assert splits == 32 and splits * rps > M + rps                 # at least one split without rows
    if M == 4225 and chunk == 64:
        assert last == 1
    check_wgrad_exact(kind, M, na, nb, "scalar" if na % 2 else "vec", M + na)


def check_cat_exact(kind, M, na, nb1, nb2, mode, seed, bias=True):
    gen = torch.Generator().manual_seed(seed)
    ta, tb = _operand_types(kind)
    A, B1 = gm.ints((M, na), gen), gm.ints((M, nb1), gen)
    a, b1 = place(A, mode, 0, ta), place(B1, mode, 1 if mode == "scalar" else 0, tb)
    b2 = place(gm.ints((M, nb2), gen), mode, 2, tb) if nb2 else None
    flat = lambda r, c: gm.embed(torch.full((r, c), NAN, device=DEV), 1, 0, 0, CANARY)
    dW1, dW2, db = flat(na, nb1), (flat(na, nb2) if nb2 else None), (flat(1, na) if bias else None)
    wgrad_cat_raw(kind, a, b1, b2, dW1, dW2, db)
    where = "%s M=%d n_a=%d n_b=%d+%d %s" % (kind, M, na, nb1, nb2, mode)
    for got, want in ((dW1, gm.ref_wgrad(a, b1)[0]), (dW2, gm.ref_wgrad(a, b2)[0] if nb2 else None), (db, gm.ref_colsum(a)[0][None, :] if bias else None)):
        if got is not None:
            assert not torch.isnan(got).any(), where
            assert torch.equal(got.double(), want), where
            assert gm.outside_intact(got, CANARY), where


@pytest.mark.parametrize("M", gm.WGRAD_M)
@pytest.mark.parametrize("kind", CAT_KERNELS)
def test_wgrad_cat_exact(kind, M):
    """the merged launches (two B matrices and the column sums of A) against fp64 -- not against the separate calls --, through the vector path
    (aligned base, row stride a multiple of 16 bytes) and the scalar path; the bias sums are exact on integers too"""
    for i, (na, nb) in enumerate(gm.WGRAD_N):
        nb2 = gm.WGRAD_N[(i + 2) % 5][1]
        for mode in ("vec", "scalar"):
            check_cat_exact(kind, M, na, nb, nb2 if (i + M) % 3 else 0, mode, M * 11 + i, bias=bool((i + M) % 4))


@pytest.mark.parametrize("M,na,nb", gm.WGRAD_CAPPED)
@pytest.mark.parametrize("kind", CAT_KERNELS)
def test_wgrad_cat_exact_where_the_splits_are_capped(kind, M, na, nb):
    check_cat_exact(kind, M, na, nb, 65, "vec" if na % 2 else "scalar", M + na)


WGRAD_RANGE = ((4100, 130, 65), (257, 65, 130), (4225, 64, 3))


@pytest.mark.parametrize("M,na,nb", WGRAD_RANGE)
@pytest.mark.parametrize("kind", ("f32", "x3", "b_ff", "b_bb", "x3_cat", "bcat_ff", "bcat_bb"))
def test_wgrad_range(kind, M, na, nb):
    """Wide-range A and B: every element of dW within max(4 e, 2^-23) * |A|^T|B| of fp64, e being the worst per-element error (same units) of a
    plain fp32 CPU matmul on the same inputs (test_gemm_model_cpu.py: 1e-7 .. 7e-7).  Both are fp32 sums of the same terms in different orders;
    the kernel's order -- row splits, then a two-level reduce -- is the shorter chain.  bf16 kernels: on the operands rounded to bf16."""
    gen = torch.Generator().manual_seed(M)
    A, B = gm.wide((M, na), gen), gm.wide((M, nb), gen)
    if kind.startswith("b"):
        A, B = gm.bf16_round(A), gm.bf16_round(B)
    ref_c, mag_c = gm.ref_wgrad(A, B)
    bound = gm.wgrad_bound((((A.t() @ B).double() - ref_c).abs() / mag_c).max().item())
    ta, tb = _operand_types(kind)
    a, b = place(A, "vec", 0, ta), place(B, "scalar", 1, tb)
    if kind.endswith("cat") or kind.startswith("bcat"):
        dW = gm.embed(torch.full((na, nb), NAN, device=DEV), 1, 0, 0, CANARY)
        db = gm.embed(torch.full((1, na), NAN, device=DEV), 1, 0, 0, CANARY)
        wgrad_cat_raw(kind, a, b, None, dW, None, db)
        s, smag = gm.ref_colsum(A)
        assert ((db[0].double().cpu() - s).abs() <= 2.0 ** -23 * smag).all()      # fp64 sums rounded once to fp32
    else:
        dW = gm.embed(torch.full((na, nb), NAN, device=DEV), 2, 0, 5, CANARY)
        wgrad_raw(kind, a, b, dW, 0)
    err = ((dW.double().cpu() - ref_c).abs() / mag_c).max().item()
    print("wgrad range %s M=%d: %.3g of |A|^T|B|, bound %.3g" % (kind, M, err, bound))
    assert gm.outside_intact(dW, CANARY) and err <= bound


# ---- locality -------------------------------------------------------------------------------------------------------------------------------------------
LOCALITY_FWD = [gm.Case("F32", "f32", 129, 65, 37, 30, ()), gm.Case("X3_SMALL", "x3", 97, 65, 37, 30, ("DGNN_X3_SMALL",)),
                gm.Case("X3_MID1", "x3", 961, 449, 301, 215, ("DGNN_GEMM_MID",)), gm.Case("X3", "x3", 129 * 128 + 1, 129, 37, 30, ()),
                gm.Case("X2H", "x2h", 8193, 129, 37, 30, ()), gm.Case("B_SMALL", "bf16", 97, 65, 37, 30, ("DGNN_BF16_SMALL",)),
                gm.Case("B", "bf16", 129 * 128 + 1, 63, 67, 62, ())]


@pytest.mark.parametrize("c", LOCALITY_FWD, ids=gm.case_id)
def test_forward_locality_of_nan_and_inf(c):
    """a NaN in one row of A1 and an Inf in one row of A2 (the last row, in the ragged tile) make those output rows non-finite and leave every
    other row at its exact value"""
    (A1, W1, A2, W2), (bias, scale, shift), ref = exact_case(c)
    A1, A2 = A1.clone(), A2.clone()
    r1, r2 = c.M // 2, c.M - 1
    A1[r1, c.k1 - 1] = NAN
    A2[r2, 0] = float("inf")
    adt = torch.bfloat16 if c.entry == "bf16" else None
    out = out_buffer(c.M, c.n_out)
    assert_variant(c, fwd_raw(c.entry, place(A1, "vec", 0, adt), place(W1, "vec", 2), place(A2, "scalar", 1, adt), place(W2, "scalar", 3), bias, scale, shift, 0, out))
    clean = torch.ones(c.M, dtype=torch.bool, device=DEV)
    clean[r1] = clean[r2] = False
    assert torch.equal(out[clean].double(), ref[clean])
    assert not torch.isfinite(out[~clean]).any()
    assert gm.outside_intact(out, CANARY)


@pytest.mark.parametrize("kind", ("f32", "x3", "b_bb", "b_ff", "x3_cat", "bcat_bb", "bcat_ff"))
def test_wgrad_locality_of_nan_and_inf(kind):
    """a NaN in column j of A (in the one-row last split) and an Inf in another column show in rows j of dW and element j of the bias sums only"""
    M, na, nb = 129, 65, 63
    gen = torch.Generator().manual_seed(5)
    A, B = gm.ints((M, na), gen), gm.ints((M, nb), gen)
    j1, j2 = 64, 7
    clean = torch.ones(na, dtype=torch.bool, device=DEV)
    clean[j1] = clean[j2] = False
    ref, _ = gm.ref_wgrad(A.to(DEV), B.to(DEV))
    A[M - 1, j1] = NAN
    A[40, j2] = float("inf")
    ta, tb = _operand_types(kind)
    a, b = place(A, "scalar", 0, ta), place(B, "vec", 0, tb)
    if "cat" in kind:
        dW, db = gm.embed(torch.full((na, nb), NAN, device=DEV), 1, 0, 0, CANARY), gm.embed(torch.full((1, na), NAN, device=DEV), 1, 0, 0, CANARY)
        wgrad_cat_raw(kind, a, b, None, dW, None, db)
        s, _ = gm.ref_colsum(gm.ints((M, na), torch.Generator().manual_seed(5)).to(DEV))
        assert torch.equal(db[0][clean].double(), s[clean]) and not torch.isfinite(db[0][~clean]).any()
    else:
        dW = gm.embed(torch.full((na, nb), NAN, device=DEV), 2, 0, 5, CANARY)
        wgrad_raw(kind, a, b, dW, 0)
    assert torch.equal(dW[clean].double(), ref[clean]) and not torch.isfinite(dW[~clean]).any()
    assert gm.outside_intact(dW, CANARY)
