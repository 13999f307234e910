"""The fused decoder (k_decoder_rows, k_decoder_fused, k_decoder_rows_bf16 in both modes) and the KL cell loss (k_kl_loss_fwd / _finalize / _bwd
and the one-launch k_kl_loss_step) at their edges; tests/decoder_loss_model.py has the references, the inputs and the sizes.

Decoder: each kernel is reached on purpose (row alignment and stride) and called through the C ABI, with y inside a NaN-filled buffer (ldy >
128) and the logits inside a canary buffer (ldo in {n_out, 3}).  Integer inputs and the bf16-part cases are compared with fp64 bit for bit at
every edge of the 32- and 64-row tiles and at the smallest M where the row kernels prefetch a further tile and k_decoder_fused loops; randn
and wide-range inputs are held per element to C_FWD_F32 / C_FWD_BF16 of the magnitude.  Measured on an MI355X, largest error / bound:
rows 0.13, fused_misaligned 0.13, fused_stride 0.13, bf16_single 0.052, bf16_comp 0.056.

Loss: saturated rows give integer sums at every block edge, range rows are bounded by B = max(4 e, 2^-23) of their magnitudes, e being the
error of the reference's fp32 op chain run with torch on the CPU on the same rows (measured: weighted sum e <= 9.4e-8; gradient e up to 2.1e-6
on the mixed rows, 5.9e-5 there with the log norm, 3.2e-7 on the fitted rows; test_decoder_loss_model_cpu.py says where they come from).
Largest kernel error / bound per norm (none / log / sqrt) on an MI355X: weighted sum 0.18 / 0.18 / 0.18, gradient 0.47 / 0.28 / 0.25, sum of
the weights (bound 2^-23) 3e-9 / 0.22 / 0.19.  The gradient bound carries an absolute fp32 underflow allowance of 2^-126
(decoder_loss_model.ref_kl).  With row terms and the log weight evaluated in plain fp32 (logf(expf + expf), logf(1.f + vol)) the single-row
batch missed both floors: 1.27 B on the weighted sum and 1.08 * 2^-23 on the weight; loss.hip now rounds each elementary function once.
The one-launch form is compared with the three-launch path bit for bit, and the overall-accuracy counter with the reference's rule on logits
that differ by less than the fp32 log-softmax resolves."""
import functools

import pytest
import torch

import decoder_loss_model as dm
import gemm_model as gm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CANARY = -(2.0 ** 24)          # exact in fp32, larger than any exact result here
E_INVALID, E_UNSUPPORTED = -1, -2


def _lib():
    from dgnn_amd._lib import lib, ptr, stream_ptr
    return lib(), ptr, stream_ptr


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _dev(d):
    return type(d)(*(None if t is None else t.to(DEV) for t in d))


# ---- decoder ----------------------------------------------------------------------------------------------------------------------------------------
def place_y(kernel, y):
    """y on the device inside a NaN-filled buffer (two rows below, columns on both sides), laid out so that `kernel` is the one dispatched"""
    y = y.to(DEV)
    if dm.is_bf16(kernel):
        v = gm.embed(y.to(torch.bfloat16), 2, 3, 2, NAN, 0, True)
        assert v.data_ptr() % 16 == 0 and v.stride(0) % 8 == 0
    elif kernel == "rows":
        v = gm.embed(y, 2, 3, 2, NAN, 0, True)
        assert v.data_ptr() % 16 == 0 and v.stride(0) % 4 == 0
    elif kernel == "fused_misaligned":
        v = gm.embed(y, 2, 3, 2, NAN, 4, True)
        assert v.data_ptr() % 16 == 4 and v.stride(0) % 4 == 0
    else:
        assert kernel == "fused_stride"
        v = gm.embed(y, 2, 3, 2, NAN, 0, False)
        assert v.data_ptr() % 16 == 0 and v.stride(0) % 4 != 0
    assert v.stride(0) > dm.K_IN
    return v


def out_buffer(M, o):
    """[M, n_out] of NaN inside a canary buffer with row stride o.ldo, two rows below"""
    v = gm.embed(torch.full((M, o.n_out), NAN, device=DEV), 2, 0, o.ldo - o.n_out, CANARY)
    assert v.stride(0) == o.ldo
    return v


def decoder_raw(kernel, y, a, out, k=dm.K_IN, hidden=dm.HID, n_out=None, M=None):
    """one call of the C entry point; -> its return code"""
    lib, ptr, stream_ptr = _lib()
    n_out = a.W3.size(0) if n_out is None else n_out
    M = y.size(0) if M is None else M
    assert a.W0.is_contiguous() and a.W3.is_contiguous() and y.stride(1) == 1 and out.stride(1) == 1
    args = (ptr(y), y.stride(0), M, k, ptr(a.W0), ptr(a.b0), ptr(a.scale), ptr(a.shift), hidden, ptr(a.W3), ptr(a.b3), n_out, ptr(out), out.stride(0))
    if dm.is_bf16(kernel):
        rc = lib.dgnn_decoder_fused_fwd_bf16(*args, dm.bf16_mode(kernel), stream_ptr())
    else:
        rc = lib.dgnn_decoder_fused_fwd(*args, stream_ptr())
    torch.cuda.synchronize()
    return rc


@functools.lru_cache(maxsize=None)
def exact_inputs(M):
    return _dev(dm.exact_decoder(M, _gen(M), tile_tag=M > 4097))


@functools.lru_cache(maxsize=None)
def exact_ref(M, n_out, b0, ss, b3):
    """fp64 logits of the integer inputs, once per option set: integers are bf16 values, so every kernel shares them"""
    ref, mag = dm.ref_decoder(*dm.with_opts(exact_inputs(M), dm.Opt(n_out, b0, ss, b3, n_out)))
    assert mag.max().item() * 2 < 2.0 ** 24
    return ref


def check_decoder_call(kernel, y, a, o, want, where):
    out = out_buffer(y.size(0), o)
    assert decoder_raw(kernel, y, a, out) == 0, where
    assert not torch.isnan(out).any(), "NaN in the logits: " + where
    assert gm.outside_intact(out, CANARY), "canary moved: " + where
    if want is not None:
        assert torch.equal(out.double(), want), "%s: max difference %g" % (where, (out.double() - want).abs().max().item())
    return out


@pytest.mark.parametrize("M", dm.DECODER_M + (dm.DECODER_M_BIG,))
@pytest.mark.parametrize("kernel", dm.DECODER_KERNELS)
def test_decoder_exact(kernel, M):
    """Integer y, W0, b0, W3, power-of-two scale, integer shift and b3: every kernel returns the fp64 logits bit for bit, with and without b0,
    scale / shift and b3, for one and two outputs, ldo = n_out and 3 -- every option set at every M up to 4097, four sets that take each branch
    both ways at the large M, where rows carry their tile's index.  The canary around the logits (with n_out = 1 and ldo = 3 too) and the NaN
    around y stay where they are, and no NaN reaches a logit: the clamped tail rows read row M - 1."""
    d = exact_inputs(M)
    y = place_y(kernel, d.y)
    for o in (dm.ALL_OPTS if M <= 4097 else dm.FEW_OPTS):
        check_decoder_call(kernel, y, dm.with_opts(d, o), o, exact_ref(M, *o[:4]), "%s M=%d %s" % (kernel, M, o))
    assert gm.outside_intact(y, NAN)


PARTS = (("rows", "y3"), ("rows", "W0_3"), ("fused_stride", "y3"), ("fused_misaligned", "W0_3"), ("bf16_comp", "W0_2"), ("bf16_single", "W0_2"))


@pytest.mark.parametrize("M", [33, 4097])
@pytest.mark.parametrize("kernel,which", PARTS)
def test_decoder_parts_exact(kernel, which, M):
    """18-bit values with non-zero bf16 hi, mid and lo parts in one column of every k-step and k-group of y (against +-1 in W0), then of W0
    (against +-2^e in y): k_decoder_rows returns the fp64 logits only if all three parts of either operand are multiplied in (the fp32-MFMA
    kernel takes the same inputs).  The bf16 decoder gets 16-bit W0 values against integer y: its compensated mode must equal fp64 on W0 = hi +
    lo, its single mode on hi alone, and the two differ.  test_decoder_loss_model_cpu.py proves the inputs exact and the parts needed."""
    d = _dev(dm.parts_decoder(M, which, _gen(M, len(which))))
    y = place_y(kernel, d.y)
    for n_out in (1, 2):
        o = dm.Opt(n_out, True, False, True, 3)
        a = dm.with_opts(d, o)
        ref, _ = dm.ref_decoder(a.y, dm.w0_as_seen(a.W0, kernel), *a[2:])
        check_decoder_call(kernel, y, a, o, ref, "%s %s M=%d n_out=%d" % (kernel, which, M, n_out))
        if which == "W0_2":
            other = dm.ref_decoder(a.y, dm.w0_as_seen(a.W0, "bf16_single" if kernel == "bf16_comp" else "bf16_comp"), *a[2:])[0]
            assert (other != ref).any(dim=1).float().mean().item() > 0.5


RANGE_WORST = {}


@pytest.mark.parametrize("kind", ["randn", "wide"])
@pytest.mark.parametrize("M", dm.DECODER_M + (dm.DECODER_M_BIG,))
@pytest.mark.parametrize("kernel", dm.DECODER_KERNELS)
def test_decoder_range(kernel, M, kind):
    """randn inputs and rows with a wide dynamic range: every logit within C * (|W3| m1 + |W3| h + |b3|) of fp64 (decoder_loss_model.ref_decoder),
    C = C_FWD_F32 for the two fp32 kernels and C_FWD_BF16 for the bf16 kernel against y as stored and W0 as its mode sees it"""
    d = _dev(dm.range_decoder(M, kind, _gen(M, len(kind))))
    y = place_y(kernel, d.y)
    C = gm.C_FWD_BF16 if dm.is_bf16(kernel) else gm.C_FWD_F32
    worst = 0.0
    for o in dm.FEW_OPTS:
        a = dm.with_opts(d, o)
        ref, mag = dm.ref_decoder(y.float(), dm.w0_as_seen(a.W0, kernel), *a[2:])
        out = check_decoder_call(kernel, y, a, o, None, "%s M=%d %s" % (kernel, M, o))
        err = ((out.double() - ref).abs() / mag).max().item()
        worst = max(worst, err / C)
        print("decoder range %s M=%d %s %s: %.3g of the magnitude, %.3g of the bound" % (kernel, M, kind, tuple(o), err, err / C))
        assert torch.isfinite(out).all() and err <= C
    RANGE_WORST[kernel] = max(RANGE_WORST.get(kernel, 0.0), worst)
    print("decoder range worst so far %s: %.3g of the bound" % (kernel, RANGE_WORST[kernel]))
    assert gm.outside_intact(y, NAN)


@pytest.mark.parametrize("kernel", ["rows", "fused_stride", "bf16_comp"])
def test_decoder_refusals_launch_nothing(kernel):
    """M = 0 is fine and writes nothing; k != 128, hidden != 64, n_out = 3, a scale without its shift and, for the bf16 entry, rows that are
    not 16-byte aligned or whose stride is no multiple of 8 are refused: the logits buffer holds its canary in every element afterwards"""
    d = exact_inputs(33)
    a = dm.with_opts(d, dm.Opt(2, True, True, True, 3))
    y = place_y(kernel, d.y)
    W3x = torch.cat([a.W3, a.W3[:1]]).contiguous()

    def call(want, **kw):
        out = gm.embed(torch.full((33, 3), CANARY, device=DEV), 2, 0, 0, CANARY)
        aa = kw.pop("a", a)
        yy = kw.pop("y", y)
        assert decoder_raw(kernel, yy, aa, out, **kw) == want, kw
        assert bool((out._base == CANARY).all()), kw

    call(0, M=0)
    call(E_UNSUPPORTED, k=127)
    call(E_UNSUPPORTED, k=64)
    call(E_UNSUPPORTED, hidden=32)
    call(E_UNSUPPORTED, n_out=3, a=a._replace(W3=W3x))
    call(E_INVALID, a=a._replace(shift=None))
    call(E_INVALID, a=a._replace(scale=None))
    call(E_INVALID, n_out=0)
    if dm.is_bf16(kernel):
        yb = d.y.to(torch.bfloat16)
        call(E_UNSUPPORTED, y=gm.embed(yb, 2, 3, 2, NAN, 4, True))
        call(E_UNSUPPORTED, y=gm.embed(yb, 2, 3, 2, NAN, 0, False))


def test_ops_decoder_entry_points_agree_with_the_raw_calls():
    """ops.decoder_fused_fwd / _bf16 (ldo = n_out, the mode of DGNN_BF16_MODE) on the integer inputs"""
    from dgnn_amd import ops
    d = exact_inputs(257)
    for o in (dm.Opt(1, True, True, True, 1), dm.Opt(2, False, False, False, 2)):
        a = dm.with_opts(d, o)
        want = exact_ref(257, *o[:4])
        assert torch.equal(ops.decoder_fused_fwd(*a).double(), want)
        assert torch.equal(ops.decoder_fused_fwd(place_y("fused_stride", d.y), *a[1:]).double(), want)
        assert torch.equal(ops.decoder_fused_fwd_bf16(d.y.to(torch.bfloat16), *a[1:]).double(), want)


# ---- loss -------------------------------------------------------------------------------------------------------------------------------------------------
def place_rows(logits, gt, vol):
    """logits as the two leading columns of [n, 3], gt of [n, 4], vol as a column of [n, 4]; NaN in every other column"""
    n = logits.size(0)
    L, G, X = (torch.full((n, c), NAN, device=DEV) for c in (3, 4, 4))
    L[:, :2], G[:, :2], X[:, 0] = logits.to(DEV), gt.to(DEV), vol.to(DEV)
    return L[:, :2], G[:, :2], X[:, 0]


def dl_buffer(n):
    v = gm.embed(torch.full((n, 2), NAN, device=DEV), 2, 0, 3, CANARY)
    assert v.stride(0) == 5
    return v


def _result():
    """(sums fp64 [3], loss fp32 0-dim) inside canary buffers"""
    s = torch.full((5,), CANARY, dtype=torch.float64, device=DEV)
    l = torch.full((3,), CANARY, device=DEV)
    return s, l


def _result_ok(s, l):
    return s[0].item() == CANARY and s[4].item() == CANARY and l[0].item() == CANARY and l[2].item() == CANARY


def loss_fwd_raw(rows, norm):
    lib, ptr, stream_ptr = _lib()
    lv, gv, vv = rows
    n = lv.size(0)
    s, l = _result()
    scratch = torch.full((int(lib.dgnn_kl_cell_loss_scratch_doubles(n)),), NAN, dtype=torch.float64, device=DEV)
    rc = lib.dgnn_kl_cell_loss_fwd(ptr(lv), lv.stride(0), ptr(gv), gv.stride(0), ptr(vv), vv.stride(0), norm, n, ptr(s[1:]), ptr(l[1:]), ptr(scratch), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and _result_ok(s, l)
    return s[1:4].clone(), l[1].clone()


def loss_bwd_raw(rows, norm, sums, grad):
    lib, ptr, stream_ptr = _lib()
    lv, gv, vv = rows
    n = lv.size(0)
    dl = dl_buffer(n)
    g = torch.tensor([grad], dtype=torch.float32, device=DEV)
    rc = lib.dgnn_kl_cell_loss_bwd(ptr(lv), lv.stride(0), ptr(gv), gv.stride(0), ptr(vv), vv.stride(0), norm, n, ptr(sums), ptr(g), ptr(dl), dl.stride(0), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and gm.outside_intact(dl, CANARY)
    return dl


def loss_step_raw(rows, norm, grad=None, running=None, backward=True):
    """-> (rc, sums, loss, dlogits | None)"""
    lib, ptr, stream_ptr = _lib()
    lv, gv, vv = rows
    n = lv.size(0)
    s, l = _result()
    dl = dl_buffer(n) if backward else None
    g = None if grad is None else torch.tensor([grad], dtype=torch.float32, device=DEV)
    rc = lib.dgnn_kl_cell_loss_step(ptr(lv), lv.stride(0), ptr(gv), gv.stride(0), ptr(vv), vv.stride(0), norm, n, ptr(g), ptr(s[1:]), ptr(l[1:]), ptr(running),
                                    ptr(dl), 5, stream_ptr())
    torch.cuda.synchronize()
    assert _result_ok(s, l) and (dl is None or gm.outside_intact(dl, CANARY))
    return rc, s[1:4].clone(), l[1].clone(), dl


def f32_quotient(sums):
    s = sums.cpu()
    return s[0].float() / s[1].float()


@pytest.mark.parametrize("n", dm.LOSS_N)
def test_loss_saturated_rows_give_integer_sums(n):
    """targets (1,0) / (0,1), logits an integer d in [128, 512] apart, integer volumes: a row's term is exactly 0 or d, so the three sums are
    the model's integers bit for bit at every edge of the waves, the blocks and the grid -- a row dropped or counted twice shows --, the loss is
    float32(sum) / float32(weights), and the one-launch form gives the same where it applies"""
    rows_cpu = dm.saturated_rows(n, _gen(n))
    want = dm.saturated_sums(*rows_cpu)
    r = dm.ref_kl(*rows_cpu, 0)
    assert r.sum_cw == want[0] and r.sum_w == want[1] and r.oa == want[2]
    rows = place_rows(*rows_cpu)
    sums, loss = loss_fwd_raw(rows, 0)
    assert torch.equal(sums.cpu(), want), (sums.cpu(), want)
    assert torch.equal(loss.cpu(), f32_quotient(want))
    rc, s2, l2, _ = loss_step_raw(rows, 0, backward=False)
    if n <= dm.STEP_MAX_ROWS:
        assert rc == 0 and torch.equal(s2.cpu(), want) and torch.equal(l2.cpu(), f32_quotient(want))
    else:
        assert rc == E_UNSUPPORTED


@functools.lru_cache(maxsize=None)
def range_case(n, kind):
    return dm.range_rows(n, kind, _gen(n, len(kind)))


LOSS_WORST = {}


@pytest.mark.parametrize("kind", ["mixed", "fitted"])
@pytest.mark.parametrize("norm", dm.NORMS)
@pytest.mark.parametrize("n", dm.LOSS_N)
def test_loss_range(n, norm, kind):
    """mixed rows (3 randn logits, differences up to +-120, targets with exact 0 and 1, targets that sum to 0.5 .. 2, a well-fitted block, vol
    over 1e-3 .. 1e3) and batches in which every row is well fitted, where the loss cancels to about 0: the weighted sum within B sum_k mu_k w_k
    and every gradient element within B of its magnitude, B = max(4 e, 2^-23) from the fp32 op chain on the CPU; the weights' sum within 2^-23
    of itself; the count equal to the model's; the loss the fp32 quotient of the two sums; two runs give the same bits"""
    rows_cpu = range_case(n, kind)
    grad = 1.7
    r = dm.ref_kl(*rows_cpu, norm, grad)
    b_sum, b_grad, e_sum, e_grad = dm.loss_bounds(*rows_cpu, norm, grad, r)
    rows = place_rows(*rows_cpu)
    sums, loss = loss_fwd_raw(rows, norm)
    dl = loss_bwd_raw(rows, norm, sums, grad)
    s = sums.cpu()
    err_sum = abs(s[0] - r.sum_cw).item() / (r.mu * r.w).sum().item()
    err_w = abs(s[1] - r.sum_w).item() / r.w.abs().sum().item()
    err_grad = dm.grad_error(dl.cpu(), r)
    w = LOSS_WORST.setdefault(norm, [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], err_sum / b_sum), max(w[1], err_grad / b_grad), max(w[2], err_w / dm.LOSS_FLOOR)
    print("loss range n=%d norm=%d %s: cpu chain %.3g / %.3g; kernel sum %.3g (%.3g of B), gradient %.3g (%.3g of B), weights %.3g (%.3g of 2^-23); worst "
          "of this norm so far %.3g %.3g %.3g" % (n, norm, kind, e_sum, e_grad, err_sum, err_sum / b_sum, err_grad, err_grad / b_grad, err_w, err_w / dm.LOSS_FLOOR, *w))
    assert not torch.isnan(dl).any()
    assert err_sum <= b_sum
    assert err_grad <= b_grad
    assert err_w <= dm.LOSS_FLOOR
    assert s[2].item() == r.oa
    assert torch.equal(loss.cpu(), f32_quotient(s))
    if kind == "fitted":
        assert abs(loss.item()) <= (b_sum * (r.mu * r.w).sum().item() / r.sum_w.item() + abs(r.loss.item())) * 1.001     # absolute: about 0
    sums2, loss2 = loss_fwd_raw(rows, norm)
    dl2 = loss_bwd_raw(rows, norm, sums2, grad)
    assert torch.equal(sums2, sums) and torch.equal(loss2, loss) and torch.equal(dl2, dl)


@pytest.mark.parametrize("norm", dm.NORMS)
@pytest.mark.parametrize("n", [n for n in dm.LOSS_N if n <= dm.STEP_MAX_ROWS])
def test_loss_one_launch_form_gives_the_bits_of_the_three_launch_path(n, norm):
    """dgnn_kl_cell_loss_step against dgnn_kl_cell_loss_fwd + _bwd on the mixed rows: sums, loss and dlogits bit for bit, with grad_loss NULL (1)
    and 1.7, without the backward, and with a preloaded `running` that ends as running + sums in fp64; two runs give the same bits"""
    rows = place_rows(*range_case(n, "mixed"))
    sums, loss = loss_fwd_raw(rows, norm)
    for grad in (None, 1.7):
        dl = loss_bwd_raw(rows, norm, sums, 1.0 if grad is None else grad)
        start = torch.tensor([1000.25, 7.5, 12345.0], dtype=torch.float64)
        runbuf = torch.full((5,), CANARY, dtype=torch.float64, device=DEV)
        runbuf[1:4] = start.to(DEV)
        for _ in range(2):
            runbuf[1:4] = start.to(DEV)
            rc, s2, l2, dl2 = loss_step_raw(rows, norm, grad, runbuf[1:4])
            assert rc == 0 and torch.equal(s2, sums) and torch.equal(l2, loss) and torch.equal(dl2, dl)
            assert torch.equal(runbuf[1:4].cpu(), start + sums.cpu()) and runbuf[0].item() == CANARY and runbuf[4].item() == CANARY
    rc, s2, l2, none = loss_step_raw(rows, norm, 1.7, None, backward=False)
    assert rc == 0 and none is None and torch.equal(s2, sums) and torch.equal(l2, loss)


def test_loss_one_launch_form_declines_beyond_its_limit():
    """65537 rows: the raw call returns DGNN_E_UNSUPPORTED and ops.kl_cell_loss_step None, nothing is launched -- sums, loss, dlogits and
    `running` keep their contents -- and ops' two-call path gives the bits of the raw calls; at 65536 rows ops gives the one-launch result"""
    from dgnn_amd import ops
    n = dm.STEP_MAX_ROWS + 1
    rows = place_rows(*range_case(n, "mixed"))
    running = torch.tensor([1000.25, 7.5, 12345.0], dtype=torch.float64, device=DEV)
    before = running.clone()
    rc, s, l, dl = loss_step_raw(rows, 1, 1.7, running)
    assert rc == E_UNSUPPORTED and bool((s == CANARY).all()) and l.item() == CANARY and torch.isnan(dl).all() and torch.equal(running, before)
    assert ops.kl_cell_loss_step(*rows, 1, running=running) is None and torch.equal(running, before)
    sums, loss = loss_fwd_raw(rows, 1)
    l2, s2 = ops.kl_cell_loss_fwd(*rows, 1)
    assert torch.equal(s2, sums) and torch.equal(l2, loss)
    g = torch.tensor(1.7, device=DEV)
    assert torch.equal(ops.kl_cell_loss_bwd(*rows, 1, sums, g), loss_bwd_raw(rows, 1, sums, 1.7))
    rows = place_rows(*range_case(dm.STEP_MAX_ROWS, "mixed"))
    sums, loss = loss_fwd_raw(rows, 1)
    l2, s2, dl2 = ops.kl_cell_loss_step(*rows, 1, running=running, grad_loss=g)
    assert torch.equal(s2, sums) and torch.equal(l2, loss) and torch.equal(dl2, loss_bwd_raw(rows, 1, sums, 1.7)) and torch.equal(running.cpu(), before.cpu() + sums.cpu())


@pytest.mark.parametrize("n", [21, 1024 + 11, 2049, dm.STEP_MAX_ROWS + 1])
def test_loss_overall_accuracy_follows_the_reference_rule(n):
    """logits that differ by 0, 1e-10, 1e-8, 1.2e-7 (and mirrored), on both sides of t0 > t1 and on t0 == t1, at the first rows, at the last
    rows and across the 1024-row boundary of a saturated batch: the count is the reference's, argmax of the fp32 log-softmax pair with the
    first index on a tie -- below 3e-8 that is class 0 where the larger logit says 1 -- in both forms"""
    base = dm.saturated_rows(n, _gen(n, 3))
    R = dm.oa_edge_rows()[0].size(0)
    for where in sorted({0, n - R, max(0, min(1024 - R // 2, n - R))}):
        logits, gt = dm.with_oa_rows(base[0], base[1], where)
        want = dm.ref_kl(logits, gt, base[2], 0).oa
        by_logit = int(((gt[:, 0] > gt[:, 1]) == (logits[:, 1] > logits[:, 0])).sum())
        assert want == by_logit + 2                         # of the six rows the logit rule gets wrong, it counts two; the reference's counts the other four
        rows = place_rows(logits, gt, base[2])
        sums, _ = loss_fwd_raw(rows, 0)
        assert sums[2].item() == want, (n, where, sums[2].item(), want)
        if n <= dm.STEP_MAX_ROWS:
            rc, s2, _, _ = loss_step_raw(rows, 0, backward=False)
            assert rc == 0 and s2[2].item() == want
