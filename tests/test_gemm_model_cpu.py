"""CPU checks of tests/gemm_model.py: the exact inputs are exact in any summation order, the wide-range inputs are fair (a plain fp32 sum
stays well inside the bounds the GPU tests hold the kernels to), and the case table covers the dispatch."""
import pytest
import torch

import gemm_model as gm


def _operands(c, gen, draw=gm.ints):
    A1, W1 = draw((c.M, c.k1), gen), draw((c.n_out, c.k1), gen)
    A2, W2 = (draw((c.M, c.k2), gen), draw((c.n_out, c.k2), gen)) if c.k2 else (None, None)
    return A1, W1, A2, W2


def _rows_subset(c, n=192):
    """the fp32 matmul of a case's first, last and a few middle rows: the values are i.i.d., so the sub-problem proves what the whole would"""
    return c if c.M <= n else c._replace(M=n)


@pytest.mark.parametrize("c", gm.CASES, ids=gm.case_id)
def test_ints_cases_are_exact_in_fp32(c):
    """every table row: a plain fp32 matmul (whatever order the BLAS takes) equals the fp64 reference exactly, epilogue included"""
    gen = torch.Generator().manual_seed(c.M + 3 * c.n_out + c.k1)
    c = _rows_subset(c)
    A1, W1, A2, W2 = _operands(c, gen)
    bias, shift = gm.ints((c.n_out,), gen), gm.ints((c.n_out,), gen)
    scale = gm.pow2((c.n_out,), gen)
    ref, mag = gm.ref_fwd(A1, W1, A2, W2, bias, scale, shift, relu=True)
    got = A1 @ W1.t() + (A2 @ W2.t() if c.k2 else 0) + bias
    got = (got * scale + shift).clamp_min(0)
    assert torch.equal(got.double(), ref)
    assert mag.max().item() < 2.0 ** 24 and ref.abs().max().item() > 0
    # the same values are exact in bf16 and fp16 storage
    assert torch.equal(A1.to(torch.bfloat16).float(), A1) and torch.equal(A1.to(torch.float16).float(), A1)


@pytest.mark.parametrize("K", [1, 31, 32])
def test_three_part_against_single_part_is_exact(K):
    """18-bit values against powers of two, at most 32 terms: every fp32 partial sum is exact, and each of the three bf16 parts is non-zero"""
    gen = torch.Generator().manual_seed(K)
    A, W = gm.three_part((70, K), gen), gm.pow2((33, K), gen)
    ref, _ = gm.ref_fwd(A, W)
    assert torch.equal((A @ W.t()).double(), ref) and torch.equal(gm.seq_sum_fp32(A, W).double(), ref)
    hi = gm.bf16_round(A)
    mid = gm.bf16_round(A - hi)
    lo = A - hi - mid
    assert (hi != 0).all() and (mid != 0).all() and (lo != 0).all() and torch.equal(gm.bf16_round(lo), lo)
    # dropping the lo part moves every output: the GPU test cannot pass on two parts
    assert ((hi + mid) @ W.t() != A @ W.t()).any()


@pytest.mark.parametrize("exps", sorted(gm.ROW_EXPS))
@pytest.mark.parametrize("c", gm.RANGE_CASES, ids=gm.case_id)
def test_wide_forward_inputs_are_fair(c, exps):
    """A plain fp32 sequential sum over [A1|A2] (the longest chain, no fp64, no pairwise tree) of the wide inputs stays within HALF the bound
    the GPU test allows the kernel (gemm_model.C_FWD_F32 = 2e-6 of the magnitude), on 48 rows x 40 columns of every range case; bf16 storage is
    measured on the operands as rounded.  Measured: 5.0e-7 .. 9.1e-7 of the magnitude (7.4e-7 at K = 2125, 9.1e-7 at K = 511: with the 2^-6..2^6
    spread per element a few terms dominate a sum, and once one of them is in, every later add rounds at its size).  The kernels' chains are
    shorter (chunks of 32 or 64, split-K groups), their dropped terms 2^-25 (x3) and 2^-22 (x2h) relative; a lost or foreign term is on average
    1 / K of the magnitude, 4.7e-4 at K = 2125."""
    ea, ew = gm.ROW_EXPS[exps]
    gen = torch.Generator().manual_seed(c.k1 + c.k2)
    c = c._replace(M=48, n_out=40)
    A1, W1 = gm.wide((c.M, c.k1), gen, ea), gm.wide((c.n_out, c.k1), gen, ew)
    A2, W2 = gm.wide((c.M, c.k2), gen, ea), gm.wide((c.n_out, c.k2), gen, ew)
    if c.entry == "bf16":
        A1, W1, A2, W2 = (gm.bf16_round(t) for t in (A1, W1, A2, W2))
    ref, mag = gm.ref_fwd(A1, W1, A2, W2)
    assert torch.isfinite(ref.float()).all() and (mag > 0).all()
    got = gm.seq_sum_fp32(torch.cat([A1, A2], 1), torch.cat([W1, W2], 1))
    err = ((got.double() - ref).abs() / mag).max().item()
    print("wide forward %s %s: fp32 sequential sum off by %.3g of the magnitude" % (gm.case_id(c), exps, err))
    assert err <= 0.5 * gm.C_FWD_F32
    # the row exponents are there: A rows at 2^+60 meet W rows at 2^-60 (or the reverse)
    if exps != "mid":
        big, small = (A1, W1) if exps == "a_big" else (W1, A1)
        assert big.abs().max().item() > 2.0 ** 60 and small.abs().max().item() < 2.0 ** -40


WGRAD_RANGE = ((4100, 130, 65), (257, 65, 130), (4225, 64, 3))


@pytest.mark.parametrize("M,na,nb", WGRAD_RANGE)
def test_wide_wgrad_inputs_and_the_cpu_error(M, na, nb):
    """The error of a plain fp32 CPU matmul A^T B on the wide inputs against fp64, per element in units of |A|^T|B|.  Measured: 1.5e-7
    (M = 4100), 7.3e-7 (M = 257), 1.05e-7 (M = 4225); on bf16-rounded operands 1.4e-7, 6.7e-7 and 0.96e-7.  The GPU test allows a kernel four
    times the figure it measures on its own inputs, and not less than 2^-23 = 1.19e-7 (gemm_model.wgrad_bound).  Here: the figure is of
    fp32-rounding size, so that the bound stays below 1e-5 -- a twentieth of one lost row's average share of a sum (1 / M = 2.4e-4 of the
    magnitude at M = 4225)."""
    gen = torch.Generator().manual_seed(M)
    A, B = gm.wide((M, na), gen), gm.wide((M, nb), gen)
    for name, (a, b) in dict(fp32=(A, B), bf16=(gm.bf16_round(A), gm.bf16_round(B))).items():
        ref, mag = gm.ref_wgrad(a, b)
        err = (((a.t() @ b).double() - ref).abs() / mag).max().item()
        print("wide wgrad M=%d %s: fp32 CPU matmul off by %.3g of |A|^T|B|" % (M, name, err))
        assert gm.WGRAD_FLOOR <= gm.wgrad_bound(err) <= 1e-5


def test_enum_mirror_and_table_cover_every_variant():
    assert gm.header_variants() == gm.VARIANTS
    reached = {c.variant for c in gm.CASES}
    assert reached == set(gm.VARIANTS) - {"NONE"}
    assert {c.variant for c in gm.RANGE_CASES} == reached


@pytest.mark.parametrize("c", list(gm.CASES) + gm.RANGE_CASES, ids=gm.case_id)
def test_table_rows_reach_their_variant_under_the_default_switches(c):
    """each row against the mirrored dispatch, and each named switch takes the variant away"""
    K = c.k1 + c.k2
    assert gm.expected_variant(c.entry, c.M, c.n_out, K) == c.variant
    for s in c.switch:
        off = gm.env_switches({s: "0"})
        assert gm.expected_variant(c.entry, c.M, c.n_out, K, off) != c.variant
    assert c.M * c.n_out <= 8269 * 1300


def test_first_row_of_a_variant_is_the_smallest_that_reaches_it():
    """a canonical row cannot shrink: one row, one column or one k less (where the dispatch has a lower limit) leaves the variant"""
    first = {}
    for c in gm.CASES:
        first.setdefault(c.variant, c)
    c = first["X3_MID1"]
    assert gm.x3_variant(c.M - 40, c.n_out, c.k1) != "X3_MID1" and gm.x3_variant(c.M, c.n_out - 64, c.k1) != "X3_MID1" and gm.x3_variant(c.M, c.n_out, c.k1 - 1) != "X3_MID1"
    c = first["X3_MID4"]
    assert gm.x3_variant(c.M, c.n_out, c.k1 - 1) == "X3_MID1"
    c = first["X3_BIG"]
    assert gm.x3_variant(8191, c.n_out, 8) != "X3_BIG" and gm.x3_variant(c.M, 1280, 8) != "X3_BIG"
    assert gm.x3_variant(16384, 65, 5) == "X3_SMALL" and gm.x3_variant(16385, 65, 5) == "X3" and gm.x3_variant(16385, 64, 5) == "X3_N64"
    assert gm.bf16_variant(16384, 65, 5) == "B_SMALL" and gm.bf16_variant(16385, 65, 5) == "B"
    assert gm.x3_variant(33, 33, 1023) == "X3_SMALL" and gm.x3_variant(33, 33, 1024) == "X3_SMALL_SPLITK"


def test_wgrad_plan_edges():
    """the split arithmetic the gradient cases rely on"""
    assert gm.wgrad_plan(4100, 1024, 32) == (32, 160, 100)        # 26 splits with rows (25 x 160 + 100), splits 26..31 empty
    assert gm.wgrad_plan(4100, 1025, 32)[:2] == (32, 160)
    assert gm.wgrad_plan(22 * 192 + 1, 1024, 64) == (32, 192, 1)   # bf16 kernels: a one-row last split, 23..31 empty
    assert gm.wgrad_plan(129, 64, 64) == (2, 128, 1) and gm.wgrad_plan(257, 64, 64) == (3, 128, 1)
    assert gm.wgrad_plan(129, 64, 32) == (2, 96, 33) and gm.wgrad_plan(128, 64, 32) == (1, 128, 128)
    assert gm.wgrad_plan(70000, 2, 32)[0] == 512


def test_embed_layout():
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    for mis in (0, 4, 8, 12):
        for m4 in (True, False):
            v = gm.embed(t, 2, 3, 2, float("nan"), misalign=mis, stride_mult4=m4)
            assert torch.equal(v, t) and v.data_ptr() % 16 == mis and (v.stride(0) % 4 == 0) == m4
            assert gm.outside_intact(v, float("nan"))
            v._base[v.storage_offset() - 1] = 1.0
            assert not gm.outside_intact(v, float("nan"))
    v = gm.embed(t.to(torch.bfloat16), 1, 1, 1, float("nan"), misalign=4, stride_mult4=True)
    assert v.data_ptr() % 16 == 4 and v.stride(0) % 8 == 0 and gm.outside_intact(v, float("nan"))
    o = gm.embed(torch.zeros(3, 4), 2, 0, 3, -777.0)
    assert o.stride(0) == 7 and gm.outside_intact(o, -777.0)
    o[2, 3] = 5.0
    assert gm.outside_intact(o, -777.0)
    o._base[o.storage_offset() + 4] = 0.0
    assert not gm.outside_intact(o, -777.0)
