"""Tensor-level wrappers over the C ABI (PyTorch is used for device memory and streams only).

Every function takes CUDA(ROCm) float32 tensors whose last dimension is contiguous, launches on the
current torch stream and returns torch tensors.  No CPU path exists: a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import DgnnError, check, lib, on_device_of, ptr, stream_ptr

DGNN_E_UNSUPPORTED = -2  # include/dgnn_hip.h


def _req(t: torch.Tensor, name: str, dtype=torch.float32, dim=None, any_stride=False):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a tensor" % name)
    if not t.is_cuda:
        raise DgnnError("%s is on %s: dgnn_amd runs on the GPU only (no CPU fallback)" % (name, t.device))
    if (t.dtype not in dtype) if isinstance(dtype, tuple) else (t.dtype != dtype):
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if dim is not None and t.dim() != dim:
        raise ValueError("%s must be %d-D, got shape %s" % (name, dim, tuple(t.shape)))
    if t.dim() == 2 and t.numel() and t.size(1) > 1 and t.stride(1) != 1 and not any_stride:   # (a single column has no column stride to speak of)
        raise ValueError("%s must have a contiguous last dimension (stride %s)" % (name, t.stride()))
    return t


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.size(0) > 1 or t.stride(0) >= t.size(1) else t.size(1)


def rows2d(t: torch.Tensor, name: str) -> torch.Tensor:
    """Returns `t` as a 2-D fp32 tensor with unit column stride (copies only when it must)."""
    _req(t, name, dim=2)
    return t


ACT = (torch.float32, torch.bfloat16)   # storage types of activations: fp32 (reference arithmetic) or bf16 (BASELINE config 3)


def _sfx(t: torch.Tensor) -> str:
    """entry-point suffix for the storage type of `t`"""
    return "_bf16" if t.dtype == torch.bfloat16 else ""


def _same(t, ref, name):
    if t is not None and t.dtype != ref.dtype:
        raise TypeError("%s must have the storage type of its companion (%s), got %s" % (name, ref.dtype, t.dtype))
    return t


def _f32(n, device):
    return torch.empty(int(max(n, 1)), dtype=torch.float32, device=device)


def _f32_work(n, device):
    """work buffer whose size changes from step to step (training blocks differ in size): rounded up to a multiple of 2M floats so
    that the caching allocator sees a handful of sizes instead of a new one every step (each miss is a hipMalloc, and those
    synchronise: the first ~300 steps of a training run were 40 % slower until its cache had filled)"""
    n = int(max(n, 1))
    return torch.empty((n + (1 << 21) - 1) >> 21 << 21, dtype=torch.float32, device=device)


# ---- plan ---------------------------------------------------------------------------------------
PLAN_HINT_AUTO, PLAN_HINT_GROUPED, PLAN_HINT_REFERENCE, PLAN_HINT_GENERIC = 0, 1, 2, 3
PLAN_HINT_GROUPED_TRUSTED = 4     # GROUPED without the device-side check / standby builder: for lists this package laid out itself (partition.build_ring_part)


@on_device_of
def plan_build(edge_index: torch.Tensor, n_key: int, by: int, hint: int = PLAN_HINT_AUTO, n_other: int = 0):
    """-> (rowptr int32 [n_key+1], other int32 [E], eid int32 [E]); see dgnn_plan_build.  `n_other`: node count of the other
    side for range checking (0 = unchecked)."""
    _req(edge_index, "edge_index", torch.int64, 2, any_stride=True)
    if edge_index.size(0) != 2:
        raise ValueError("edge_index must be an int64 [2,E] tensor (any strides; the transposed [E,2] view is read in place)")
    E = edge_index.size(1)
    dev = edge_index.device
    rowptr = torch.empty(n_key + 1, dtype=torch.int32, device=dev)
    other = torch.empty(max(E, 1), dtype=torch.int32, device=dev)[:E]
    eid = torch.empty(max(E, 1), dtype=torch.int32, device=dev)[:E]
    scratch = torch.empty(int(lib().dgnn_plan_scratch_elems(E, n_key)), dtype=torch.int32, device=dev)
    check(lib().dgnn_plan_build(ptr(edge_index), edge_index.stride(0), edge_index.stride(1), E, n_key, int(n_other), by, hint, ptr(rowptr), ptr(other), ptr(eid), ptr(scratch), stream_ptr()),
          "dgnn_plan_build", poll=True)
    return rowptr, other, eid


@on_device_of
def gather_rows(src: torch.Tensor, idx: torch.Tensor, cols: int = None) -> torch.Tensor:
    """out = src[idx, :cols] (cols None: all columns); only the requested columns are read"""
    if src.dtype in (torch.bfloat16, torch.int16):   # rows of 16-bit pairs (bf16, or unsigned rows in their int16 container) move as fp32 words (bit copies)
        if not src.is_contiguous() or src.size(1) % 2 or (cols is not None and cols % 2):
            raise ValueError("16-bit gather_rows needs contiguous rows of even width")
        return gather_rows(src.view(torch.float32), idx, None if cols is None else cols // 2).view(src.dtype)
    _req(src, "src", dim=2)
    _req(idx, "idx", torch.int32, 1)
    cols = src.size(1) if cols is None else int(cols)
    if not 0 < cols <= src.size(1):
        raise ValueError("cols=%d outside (0, %d]" % (cols, src.size(1)))
    out = torch.empty((idx.numel(), cols), dtype=torch.float32, device=src.device)
    check(lib().dgnn_gather_rows_f32(ptr(src), _ld(src), ptr(idx), idx.numel(), cols, ptr(out), cols, stream_ptr()),
          "dgnn_gather_rows_f32")
    return out


@on_device_of
def scatter_rows_(out: torch.Tensor, idx: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    if src.dtype in (torch.bfloat16, torch.int16):   # bit copies of 16-bit pairs as fp32 words
        if not (src.is_contiguous() and out.is_contiguous()) or src.size(1) % 2 or out.dtype != src.dtype:
            raise ValueError("16-bit scatter_rows_ needs contiguous rows of even width and one row format")
        scatter_rows_(out.view(torch.float32), idx, src.view(torch.float32))
        return out
    _req(src, "src", dim=2)
    _req(out, "out", dim=2)
    _req(idx, "idx", torch.int64, 1)
    check(lib().dgnn_scatter_rows_f32(ptr(src), _ld(src), ptr(idx), idx.numel(), src.size(1), ptr(out), _ld(out), stream_ptr()),
          "dgnn_scatter_rows_f32")
    return out


@on_device_of
def relu(x: torch.Tensor) -> torch.Tensor:
    _req(x, "x", ACT)
    x = x.contiguous()
    y = torch.empty_like(x)
    check(getattr(lib(), "dgnn_relu" + _sfx(x))(ptr(x), x.numel(), ptr(y), stream_ptr()), "dgnn_relu")
    return y


@on_device_of
def relu_bwd(y: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    _req(y, "y", ACT)
    _same(_req(g, "g", ACT), y, "g")
    y, g = y.contiguous(), g.contiguous()
    out = torch.empty_like(g)
    check(getattr(lib(), "dgnn_relu_bwd" + _sfx(y))(ptr(y), ptr(g), g.numel(), ptr(out), stream_ptr()), "dgnn_relu_bwd")
    return out


# ---- aggregation --------------------------------------------------------------------------------
@on_device_of
def aggregate_fwd(rowptr, src, eid, n_dst, x_src, edge_attr=None, We=None, be=None, phi=None, want_phi=False):
    _req(x_src, "x_src", ACT, dim=2)
    c_in = x_src.size(1)
    a = torch.empty((n_dst, c_in), dtype=x_src.dtype, device=x_src.device)
    phi_out = None
    f_e = 0
    if We is not None:
        _req(edge_attr, "edge_attr", dim=2)
        _req(We, "We", dim=2)
        We = We.contiguous()
        be = _req(be, "be").contiguous()
        f_e = We.size(1)
        if We.size(0) != c_in or edge_attr.size(1) < f_e:
            raise ValueError("lin_e weight %s does not match c_in=%d / edge_attr %s" % (tuple(We.shape), c_in, tuple(edge_attr.shape)))
        if want_phi:
            phi_out = torch.empty((edge_attr.size(0), c_in), dtype=x_src.dtype, device=x_src.device)
    elif phi is not None:
        _same(_req(phi, "phi", ACT, dim=2), x_src, "phi")
    check(getattr(lib(), "dgnn_sage_aggregate_fwd" + _sfx(x_src))(
        ptr(rowptr), ptr(src), ptr(eid), n_dst, ptr(x_src), _ld(x_src), c_in,
        ptr(edge_attr) if We is not None else None, _ld(edge_attr) if We is not None else 0, f_e,
        ptr(We), ptr(be), ptr(phi), _ld(phi) if phi is not None else 0,
        ptr(phi_out), c_in, ptr(a), c_in, stream_ptr()), "dgnn_sage_aggregate_fwd")
    return (a, phi_out) if want_phi else a


@on_device_of
def aggregate_bwd(t_rowptr, t_dst, t_eid, n_src, rowptr_dst, x_src, da, edge_attr=None, We=None, be=None, phi=None,
                  need_dx=True):
    """-> (dx_src | None, dWe | None, dbe | None, dphi | None)"""
    _req(x_src, "x_src", ACT, dim=2)
    _same(_req(da, "da", ACT, dim=2), x_src, "da")
    _same(phi, x_src, "phi")
    c_in = x_src.size(1)
    dev = x_src.device
    dx = torch.empty((n_src, c_in), dtype=x_src.dtype, device=dev) if need_dx else None
    dWe = dbe = dphi = None
    f_e = 0
    partials = None
    if We is not None:
        We = We.contiguous()
        be = be.contiguous()
        f_e = We.size(1)
        dWe = torch.empty_like(We)     # written, not accumulated, by the slab reduction
        dbe = torch.empty_like(be)
        partials = _f32(lib().dgnn_sage_aggregate_bwd_scratch_elems(n_src, c_in, f_e), dev)
    elif phi is not None:
        dphi = torch.zeros((phi.size(0), c_in), dtype=x_src.dtype, device=dev)
    check(getattr(lib(), "dgnn_sage_aggregate_bwd" + _sfx(x_src))(
        ptr(t_rowptr), ptr(t_dst), ptr(t_eid), n_src, ptr(rowptr_dst), ptr(x_src), _ld(x_src), c_in,
        ptr(edge_attr) if We is not None else None, _ld(edge_attr) if We is not None else 0, f_e, ptr(We), ptr(be),
        ptr(phi), _ld(phi) if phi is not None else 0, ptr(da), _ld(da), ptr(dx), c_in, ptr(dWe), ptr(dbe), ptr(dphi), c_in,
        ptr(partials), stream_ptr()), "dgnn_sage_aggregate_bwd")
    return dx, dWe, dbe, dphi


# ---- dense --------------------------------------------------------------------------------------
@on_device_of
def linear_fwd(A1, W1, A2=None, W2=None, bias=None, scale=None, shift=None, relu=False, out=None, out_dtype=None):
    """out = act((A1.W1^T + A2.W2^T + bias) * scale + shift).  fp32 operands: fp32 MFMA, fp32 out.  bf16 operands (bf16 storage
    path): bf16 MFMA with fp32 accumulation, `out_dtype` bf16 (default) or fp32 (logits); an fp32 A next to bf16 storage (a
    gradient of fp32 logits) is rounded to bf16 first."""
    _req(A1, "A1", ACT, dim=2)
    W1 = _req(W1, "W1", dim=2).contiguous()
    M, n_out = A1.size(0), W1.size(0)
    if W1.size(1) != A1.size(1):
        raise ValueError("W1 %s does not match A1 %s" % (tuple(W1.shape), tuple(A1.shape)))
    if A2 is not None:
        _same(_req(A2, "A2", ACT, dim=2), A1, "A2")
        W2 = _req(W2, "W2", dim=2).contiguous()
        if A2.size(0) != M or W2.size(0) != n_out or W2.size(1) != A2.size(1):
            raise ValueError("second operand shapes do not match")
    bf = A1.dtype == torch.bfloat16
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else A1.dtype
    if not bf and out_dtype != torch.float32:
        raise TypeError("fp32 operands produce fp32 output")
    if out is None:
        out = torch.empty((M, n_out), dtype=out_dtype, device=A1.device)
    elif out.size(0) < M or out.size(1) != n_out or out.stride(0) != n_out or out.dtype != out_dtype:
        raise ValueError("out must be a contiguous [>= M, n_out] buffer of the output type")
    if bf:
        check(lib().dgnn_linear_fwd_bf16(
            ptr(A1), _ld(A1), A1.size(1), ptr(W1), W1.size(1),
            ptr(A2), _ld(A2) if A2 is not None else 0, A2.size(1) if A2 is not None else 0, ptr(W2), W2.size(1) if W2 is not None else 0,
            ptr(bias), ptr(scale), ptr(shift), int(bool(relu)), M, n_out, ptr(out), n_out, int(out_dtype == torch.float32), stream_ptr()),
            "dgnn_linear_fwd_bf16")
        return out
    # fp32 operands: bit-faithful fp32 MFMA ("f32" mode) or the fused layers' exact-split bf16 arithmetic (fp32-class, 6/16 of the time)
    if GEMM_MODE == GEMM_F16X2 and M >= 8192 and n_out > 256:  # (at n_out <= 256 the extra pass over A for the row scales costs what the products save)
        # the wide conv layers in the fused layers' fp16 two-part form (X2HP: see above)
        k1, k2 = A1.size(1), (A2.size(1) if A2 is not None else 0)
        if X2HP:
            scratch = torch.empty(int(lib().dgnn_linear_fwd_x2hp_scratch_elems(M, n_out, k1, k2)), dtype=torch.float32, device=A1.device)
            entry, name = lib().dgnn_linear_fwd_x2hp, "dgnn_linear_fwd_x2hp"
        else:
            scratch = torch.empty(int(lib().dgnn_linear_fwd_x2h_scratch_elems(M, n_out)), dtype=torch.float32, device=A1.device)
            entry, name = lib().dgnn_linear_fwd_x2h, "dgnn_linear_fwd_x2h"
        rc = entry(
            ptr(A1), _ld(A1), k1, ptr(W1), W1.size(1),
            ptr(A2), _ld(A2) if A2 is not None else 0, k2, ptr(W2), W2.size(1) if W2 is not None else 0,
            ptr(bias), ptr(scale), ptr(shift), int(bool(relu)), M, n_out, ptr(out), n_out, ptr(scratch), stream_ptr())
        if rc != DGNN_E_UNSUPPORTED:
            check(rc, name)
            return out
    fn = lib().dgnn_linear_fwd if GEMM_MODE == GEMM_F32 else lib().dgnn_linear_fwd_x3
    check(fn(
        ptr(A1), _ld(A1), A1.size(1), ptr(W1), W1.size(1),
        ptr(A2), _ld(A2) if A2 is not None else 0, A2.size(1) if A2 is not None else 0, ptr(W2), W2.size(1) if W2 is not None else 0,
        ptr(bias), ptr(scale), ptr(shift), int(bool(relu)), M, n_out, ptr(out), n_out, stream_ptr()), "dgnn_linear_fwd")
    return out


@on_device_of
def linear_wgrad(A, B):
    """dW[n_a,n_b] = A^T . B  (A [M,n_a], B [M,n_b])"""
    _req(A, "A", ACT, dim=2)
    _req(B, "B", ACT, dim=2)
    M, na, nb = A.size(0), A.size(1), B.size(1)
    dW = torch.empty((na, nb), dtype=torch.float32, device=A.device)
    if M == 0:
        return dW.zero_()
    partials = _f32(lib().dgnn_linear_wgrad_scratch_elems(M, na, nb), A.device)
    if A.dtype == torch.bfloat16 or B.dtype == torch.bfloat16:   # bf16 storage path: bf16 MFMA, fp32 gradient
        check(lib().dgnn_linear_wgrad_bf16(ptr(A), int(A.dtype == torch.float32), _ld(A), na, ptr(B), int(B.dtype == torch.float32), _ld(B), nb,
                                           M, ptr(dW), nb, 0, ptr(partials), stream_ptr()), "dgnn_linear_wgrad_bf16")
        return dW
    fn = lib().dgnn_linear_wgrad if GEMM_MODE == GEMM_F32 else lib().dgnn_linear_wgrad_x3
    check(fn(ptr(A), _ld(A), na, ptr(B), _ld(B), nb, M, ptr(dW), nb, 0, ptr(partials), stream_ptr()), "dgnn_linear_wgrad")
    return dW


@on_device_of
def linear_fwd_with_batch_stats(A1, W1, A2=None, W2=None, bias=None, gamma=None, beta=None, eps=1e-5):
    """z = A1 . W1^T + A2 . W2^T + bias and the BatchNorm batch statistics of z from the GEMM's own epilogue (dgnn_linear_fwd_x3_stats +
    dgnn_bn_stats_finalize_fold) -> (z, mean, var, scale, shift), or None where the GEMM takes the tile without that epilogue."""
    _req(A1, "A1", dim=2)
    M, n_out = A1.size(0), W1.size(0)
    z = torch.empty((M, n_out), dtype=torch.float32, device=A1.device)
    scratch = _f32(lib().dgnn_colstats_scratch_elems(M, n_out) + 2, A1.device)
    cs = (scratch.data_ptr() + 7) & ~7
    W1 = W1.contiguous()
    W2 = W2.contiguous() if W2 is not None else None
    rc = lib().dgnn_linear_fwd_x3_stats(ptr(A1), _ld(A1), A1.size(1), ptr(W1), W1.size(1), ptr(A2), _ld(A2) if A2 is not None else 0,
                                        A2.size(1) if A2 is not None else 0, ptr(W2), W2.size(1) if W2 is not None else 0, ptr(bias), M, n_out, ptr(z), n_out,
                                        cs, stream_ptr())
    if rc == DGNN_E_UNSUPPORTED:
        return None
    check(rc, "dgnn_linear_fwd_x3_stats")
    st = torch.empty((4, n_out), dtype=torch.float32, device=A1.device)
    check(lib().dgnn_bn_stats_finalize_fold(cs, (M + 31) // 32, M, n_out, ptr(st[0]), ptr(st[1]), None, None, 0.0, ptr(gamma), ptr(beta), eps, ptr(st[2]),
                                            ptr(st[3]), stream_ptr()), "dgnn_bn_stats_finalize_fold")
    return z, st[0], st[1], st[2], st[3]


@on_device_of
def linear_wgrad_cat(A, B1, B2=None, bias=True):
    """(dW1 = A^T . B1, dW2 = A^T . B2 | None, column sums of A | None) from one launch pair (dgnn_linear_wgrad_x3_cat; fp32, x3 arithmetic)"""
    _req(A, "A", dim=2)
    _req(B1, "B1", dim=2)
    M, na, nb1 = A.size(0), A.size(1), B1.size(1)
    nb2 = B2.size(1) if B2 is not None else 0
    dW1 = torch.empty((na, nb1), dtype=torch.float32, device=A.device)
    dW2 = torch.empty((na, nb2), dtype=torch.float32, device=A.device) if B2 is not None else None
    db = torch.empty(na, dtype=torch.float32, device=A.device) if bias else None
    scratch = _f32(lib().dgnn_linear_wgrad_cat_scratch_elems(M, na, nb1, nb2), A.device)
    check(lib().dgnn_linear_wgrad_x3_cat(ptr(A), _ld(A), na, ptr(B1), _ld(B1), nb1, ptr(B2), _ld(B2) if B2 is not None else 0, nb2, M, ptr(dW1), ptr(dW2),
                                         ptr(db), ptr(scratch), stream_ptr()), "dgnn_linear_wgrad_x3_cat")
    return dW1, dW2, db


@on_device_of
def aggregate_bwd_add(t_rowptr, t_dst, t_eid, n_src, rowptr_dst, x_src, da, edge_attr, We, be, add):
    """aggregate_bwd (fused 20-attribute filter) with dx[:add.size(0)] += add folded into the store -> (dx, dWe, dbe)"""
    _req(x_src, "x_src", dim=2)
    c_in = x_src.size(1)
    dx = torch.empty((n_src, c_in), dtype=torch.float32, device=x_src.device)
    We, be = We.contiguous(), be.contiguous()
    dWe, dbe = torch.empty_like(We), torch.empty_like(be)
    partials = _f32(lib().dgnn_sage_aggregate_bwd_scratch_elems(n_src, c_in, We.size(1)), x_src.device)
    check(lib().dgnn_sage_aggregate_bwd_add(ptr(t_rowptr), ptr(t_dst), ptr(t_eid), n_src, ptr(rowptr_dst), ptr(x_src), _ld(x_src), c_in, ptr(edge_attr),
                                            _ld(edge_attr), We.size(1), ptr(We), ptr(be), ptr(da), _ld(da), ptr(dx), c_in, ptr(add), _ld(add), add.size(0),
                                            ptr(dWe), ptr(dbe), ptr(partials), stream_ptr()), "dgnn_sage_aggregate_bwd_add")
    return dx, dWe, dbe


@on_device_of
def colsum(x):
    _req(x, "x", ACT, dim=2)
    out = torch.empty(x.size(1), dtype=torch.float32, device=x.device)
    if x.size(0) == 0:
        return out.zero_()
    scratch = _f32(lib().dgnn_colstats_scratch_elems(x.size(0), x.size(1)), x.device)
    check(getattr(lib(), "dgnn_colsum" + _sfx(x))(ptr(x), _ld(x), x.size(0), x.size(1), ptr(out), 0, ptr(scratch), stream_ptr()), "dgnn_colsum")
    return out


# ---- batch norm ---------------------------------------------------------------------------------
@on_device_of
def bn_fold(gamma, beta, mean, var, eps):
    c = mean.numel()
    scale = torch.empty(c, dtype=torch.float32, device=mean.device)
    shift = torch.empty(c, dtype=torch.float32, device=mean.device)
    check(lib().dgnn_bn_fold(ptr(gamma), ptr(beta), ptr(mean), ptr(var), float(eps), c, ptr(scale), ptr(shift), stream_ptr()),
          "dgnn_bn_fold")
    return scale, shift


def _written_behind_torch(*tensors):
    """the library wrote these through raw addresses: bump their version counters so that anything cached against them (the eval-mode BatchNorm
    folds, prepared parameters) is rebuilt"""
    ts = [t for t in tensors if t is not None]
    if ts:
        torch.autograd.graph.increment_version(ts)


@on_device_of
def bn_batch_stats(x, running_mean=None, running_var=None, momentum=0.1):
    _req(x, "x", ACT, dim=2)
    M, c = x.shape
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    var = torch.empty(c, dtype=torch.float32, device=x.device)
    scratch = _f32(lib().dgnn_colstats_scratch_elems(M, c), x.device)
    check(getattr(lib(), "dgnn_bn_batch_stats" + _sfx(x))(ptr(x), _ld(x), M, c, ptr(mean), ptr(var), ptr(running_mean), ptr(running_var),
                                    float(momentum), ptr(scratch), stream_ptr()), "dgnn_bn_batch_stats")
    _written_behind_torch(running_mean, running_var)
    return mean, var


@on_device_of
def scale_shift_act(x, scale, shift, relu):
    _req(x, "x", ACT, dim=2)
    y = torch.empty((x.size(0), x.size(1)), dtype=x.dtype, device=x.device)
    check(getattr(lib(), "dgnn_scale_shift_act" + _sfx(x))(ptr(x), _ld(x), ptr(scale), ptr(shift), int(bool(relu)), x.size(0), x.size(1), ptr(y),
                                     x.size(1), stream_ptr()), "dgnn_scale_shift_act")
    return y


@on_device_of
def bn_relu_bwd(x, y, dy, gamma, mean, var, eps, train, relu):
    _req(x, "x", ACT, dim=2)
    _same(_req(dy, "dy", ACT, dim=2), x, "dy")
    _same(y, x, "y")
    M, c = x.shape
    dx = torch.empty((M, c), dtype=x.dtype, device=x.device)
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
    scratch = _f32(lib().dgnn_colstats_scratch_elems(M, c), x.device)
    check(getattr(lib(), "dgnn_bn_relu_bwd" + _sfx(x))(ptr(x), _ld(x), ptr(y), _ld(y) if y is not None else 0, ptr(dy), _ld(dy), ptr(gamma), ptr(mean),
                                 ptr(var), float(eps), int(bool(train)), int(bool(relu)), M, c, ptr(dx), c, ptr(dgamma), ptr(dbeta),
                                 ptr(scratch), stream_ptr()), "dgnn_bn_relu_bwd")
    return dx, dgamma, dbeta


@on_device_of
def bn_relu_bwd_sums(x, y, dy, mean, var, eps, relu):
    """local [2, c] = (sum g, sum g * x_hat), g = dy behind the ReLU mask of y -- the half of bn_relu_bwd a partitioned scene all-reduces"""
    _req(x, "x", dim=2)
    M, c = x.shape
    sums = torch.empty((2, c), dtype=torch.float32, device=x.device)
    scratch = _f32(lib().dgnn_colstats_scratch_elems(M, c), x.device)
    check(lib().dgnn_bn_relu_bwd_sums(ptr(x), _ld(x), ptr(y), _ld(y) if y is not None else 0, ptr(dy), _ld(dy), ptr(mean), ptr(var), float(eps),
                                      int(bool(relu)), M, c, ptr(sums), ptr(scratch), stream_ptr()), "dgnn_bn_relu_bwd_sums")
    return sums


@on_device_of
def bn_relu_bwd_apply(x, y, dy, gamma, mean, var, eps, relu, sums, count):
    """dx of y = relu(bn(x)) from sums [2, c] taken over `count` rows (all ranks' rows of a partitioned scene)"""
    _req(x, "x", dim=2)
    M, c = x.shape
    dx = torch.empty((M, c), dtype=torch.float32, device=x.device)
    check(lib().dgnn_bn_relu_bwd_apply(ptr(x), _ld(x), ptr(y), _ld(y) if y is not None else 0, ptr(dy), _ld(dy), ptr(gamma), ptr(mean), ptr(var), float(eps),
                                       int(bool(relu)), M, c, ptr(sums.contiguous()), float(count), ptr(dx), c, stream_ptr()), "dgnn_bn_relu_bwd_apply")
    return dx


# ---- graph LayerNorm (csrc/lnorm.hip) -----------------------------------------------------------
def _f64_view(buf):
    """8-byte aligned address inside an fp32 work buffer"""
    return (buf.data_ptr() + 7) & ~7


@on_device_of
def graph_ln_stats(x):
    """standalone statistics pass over x [M, c] -> (fp32 work buffer holding the fp64 partials [nblk][2], nblk)"""
    _req(x, "x", dim=2)
    M, c = x.shape
    nblk = int(lib().dgnn_graph_ln_stats_blocks(M, c))
    buf = _f32(4 * max(nblk, 1) + 2, x.device)
    check(lib().dgnn_graph_ln_stats(ptr(x), _ld(x), M, c, _f64_view(buf), stream_ptr()), "dgnn_graph_ln_stats")
    return buf, nblk


@on_device_of
def graph_ln_finalize(partials_addr, nblk, pc, M, c, weight, bias, eps, device):
    """(m, sigma, r, M c) and the per-channel fold scale = w r, shift = b - m w r from partial sums [nblk][2][pc] at `partials_addr`
    -> (stats [4], scale [c], shift [c])"""
    out = torch.empty((2 * c + 4,), dtype=torch.float32, device=device)
    work = _f32(2 * 512 + 2, device)
    stats, scale, shift = out[:4], out[4:4 + c], out[4 + c:]
    if M > 0:
        check(lib().dgnn_graph_ln_finalize_fold(partials_addr, nblk, pc, M, c, ptr(weight), ptr(bias), float(eps), ptr(stats), ptr(scale), ptr(shift),
                                                _f64_view(work), stream_ptr()), "dgnn_graph_ln_finalize_fold")
    return stats, scale, shift


@on_device_of
def graph_ln_apply(x, stats, scale, bias, relu, out=None):
    """y = act((x - m) * scale + bias) -- the apply of graph_ln_finalize's fold"""
    _req(x, "x", dim=2)
    M, c = x.shape
    y = torch.empty((M, c), dtype=torch.float32, device=x.device) if out is None else out
    check(lib().dgnn_graph_ln_apply(ptr(x), _ld(x), M, c, ptr(stats), ptr(scale), ptr(bias), int(bool(relu)), ptr(y), _ld(y) if M else c, stream_ptr()),
          "dgnn_graph_ln_apply")
    return y


def graph_ln_forward(x, weight, bias, eps, relu):
    """act(LayerNorm(x)) with the standalone statistics pass -> (y, stats, scale)"""
    M, c = x.shape
    buf, nblk = graph_ln_stats(x)
    stats, scale, _ = graph_ln_finalize(_f64_view(buf), nblk, 1, M, c, weight, bias, eps, x.device)
    return graph_ln_apply(x, stats, scale, bias, relu), stats, scale


@on_device_of
def linear_fwd_ln(A1, W1, A2=None, W2=None, bias=None, weight=None, ln_bias=None, eps=1e-5, relu=True):
    """relu(LayerNorm(A1 . W1^T + A2 . W2^T + bias)): the statistics come from the GEMM's own epilogue (dgnn_linear_fwd_x3_stats colstats) where it
    takes the shape, from the standalone pass over z otherwise.  -> (y, z, stats, scale)"""
    _req(A1, "A1", dim=2)
    M, n_out = A1.size(0), W1.size(0)
    z = None
    if M > 0:
        z = torch.empty((M, n_out), dtype=torch.float32, device=A1.device)
        scratch = _f32(lib().dgnn_colstats_scratch_elems(M, n_out) + 2, A1.device)
        cs = _f64_view(scratch)
        W1c = W1.contiguous()
        W2c = W2.contiguous() if W2 is not None else None
        rc = lib().dgnn_linear_fwd_x3_stats(ptr(A1), _ld(A1), A1.size(1), ptr(W1c), W1c.size(1), ptr(A2), _ld(A2) if A2 is not None else 0,
                                            A2.size(1) if A2 is not None else 0, ptr(W2c), W2c.size(1) if W2c is not None else 0, ptr(bias), M, n_out,
                                            ptr(z), n_out, cs, stream_ptr())
        if rc != DGNN_E_UNSUPPORTED:
            check(rc, "dgnn_linear_fwd_x3_stats")
            stats, scale, _ = graph_ln_finalize(cs, (M + 31) // 32, n_out, M, n_out, weight, ln_bias, eps, A1.device)
            return graph_ln_apply(z, stats, scale, ln_bias, relu, out=z), None, stats, scale
    z = linear_fwd(A1, W1, A2, W2, bias)
    y, stats, scale = graph_ln_forward(z, weight, ln_bias, eps, relu)
    return y, z, stats, scale


@on_device_of
def graph_ln_relu_bwd(x, dy, stats, weight, scale, bias, relu):
    """backward of y = act(LayerNorm(x)) -> (dx, dweight, dbias)"""
    _req(x, "x", dim=2)
    _req(dy, "dy", dim=2)
    M, c = x.shape
    dx = torch.empty((M, c), dtype=torch.float32, device=x.device)
    dw = torch.zeros(c, dtype=torch.float32, device=x.device)
    db = torch.zeros(c, dtype=torch.float32, device=x.device)
    if M == 0:
        return dx, dw, db
    scratch = _f32(lib().dgnn_graph_ln_scratch_elems(M, c), x.device)
    check(lib().dgnn_graph_ln_relu_bwd(ptr(x), _ld(x), ptr(dy), _ld(dy), ptr(stats), ptr(weight), ptr(scale), ptr(bias), int(bool(relu)), M, c, ptr(dx), c,
                                       ptr(dw), ptr(db), ptr(scratch), stream_ptr()), "dgnn_graph_ln_relu_bwd")
    return dx, dw, db


# ---- wide conv layers on split rows (csrc/wide.hip) ---------------------------------------------
# DGNN_WIDE_SR=0: the layers wider than the fused kernels keep the fp32 aggregate + x2h / x3 GEMM pair of rounds 2-4
WIDE_SR = __import__("os").environ.get("DGNN_WIDE_SR", "1") != "0"


class SplitRows:
    """A wide activation [n, C] as the wide kernels store it (include/dgnn_hip.h "SPLIT ROWS"): `data` uint8 [n, C * 4] -- per 32 channels a 128-byte chunk
    [hi x 32 | lo x 32] fp16 of x * s in the chunk's position order -- and `scales` fp32 [n, ceil(C / 256)], one power of two per row and 256 channels.
    Produced by aggregate_sr / linear_sr / pack_rows; `.float()` gives the fp32 rows back (22 significand bits per value)."""

    def __init__(self, data, scales, channels):
        self.data, self.scales, self.channels = data, scales, int(channels)

    size = lambda self, d=None: (self.data.size(0), self.channels) if d is None else (self.data.size(0), self.channels)[d]
    shape = property(lambda self: (self.data.size(0), self.channels))
    device = property(lambda self: self.data.device)
    dtype = "split_rows"
    is_cuda = property(lambda self: self.data.is_cuda)

    def __getitem__(self, sl):
        """row ranges only (a prefix / sub-range of the rows): views of both tensors"""
        if not isinstance(sl, slice) or sl.step not in (None, 1):
            raise TypeError("SplitRows supports contiguous row ranges only")
        return SplitRows(self.data[sl], self.scales[sl], self.channels)

    def float(self):
        return unpack_rows(self)


def sr_groups(c):
    return (int(c) + 255) // 256


@on_device_of
def pack_rows(A1, A2=None, per_row=False):
    """fp32 rows [n, k1] (| [n, k2]) -> SplitRows of [A1 | A2] (widths multiples of 32); per_row: ONE scale per row (weights) instead of one per 256 channels"""
    _req(A1, "A1", dim=2)
    n, k1 = A1.shape
    k2 = 0
    if A2 is not None:
        _req(A2, "A2", dim=2)
        k2 = A2.size(1)
    C_ = k1 + k2
    if k1 % 32 or k2 % 32:
        raise ValueError("split rows need widths that are multiples of 32")
    ng = 1 if per_row else max(1, (C_ // 32 + 7) // 8)
    data = torch.empty((n, C_ * 4), dtype=torch.uint8, device=A1.device)
    scales = torch.empty((n, ng), dtype=torch.float32, device=A1.device)
    check(lib().dgnn_sr_pack(ptr(A1), _ld(A1), k1, ptr(A2), _ld(A2) if A2 is not None else 0, k2, n, 0 if per_row else 8, ptr(data), C_ * 4, ptr(scales), ng,
                             stream_ptr()), "dgnn_sr_pack")
    return SplitRows(data, scales, C_)


@on_device_of
def unpack_rows(sr: "SplitRows") -> torch.Tensor:
    n, C_ = sr.size()
    out = torch.empty((n, C_), dtype=torch.float32, device=sr.device)
    ng = sr.scales.size(1)
    gch = 8 if ng == sr_groups(C_) and not (ng == 1 and C_ > 256) else 0
    check(lib().dgnn_sr_unpack(ptr(sr.data), sr.data.stride(0), ptr(sr.scales), ng, gch, C_, n, ptr(out), C_, stream_ptr()), "dgnn_sr_unpack")
    return out


def wide_layer_supported(c_in: int, c_out: int, f_e: int) -> bool:
    """dgnn_sage_aggregate_sr + dgnn_linear_sr take this conv layer (default arithmetic only)"""
    return WIDE_SR and GEMM_MODE == GEMM_F16X2 and f_e == 20 and c_in in (128, 256, 512) and c_out % 256 == 0 and c_out > 0


@on_device_of
def sr_prepare_filter(We, be):
    c = We.size(0)
    nb = int(lib().dgnn_sr_filter_prepared_bytes(c))
    if nb <= 0 or We.size(1) != 20:
        return None
    buf = torch.empty(nb, dtype=torch.uint8, device=We.device)
    check(lib().dgnn_sr_prepare_filter(ptr(We.contiguous()), ptr(be.contiguous()), c, ptr(buf), stream_ptr()), "dgnn_sr_prepare_filter")
    return buf


@on_device_of
def aggregate_sr(rowptr, src, eid, n_dst, x, edge_attr, We, be, prep, own_rows=False):
    """-> a (SplitRows [n_dst, C]) [, x[:n_dst] as SplitRows when `own_rows` and x is an fp32 tensor] or None when the library declines the layout"""
    sr_in = isinstance(x, SplitRows)
    c = x.size(1)
    dev = x.device
    ng = sr_groups(c)
    a = SplitRows(torch.empty((n_dst, c * 4), dtype=torch.uint8, device=dev), torch.empty((n_dst, ng), dtype=torch.float32, device=dev), c)
    xo = None
    if own_rows and not sr_in:
        xo = SplitRows(torch.empty((n_dst, c * 4), dtype=torch.uint8, device=dev), torch.empty((n_dst, ng), dtype=torch.float32, device=dev), c)
    if sr_in:
        xp, ldx, xs = ptr(x.data), x.data.stride(0), ptr(x.scales)
    else:
        _req(x, "x", dim=2)
        xp, ldx, xs = ptr(x), _ld(x), None
    rc = lib().dgnn_sage_aggregate_sr(ptr(rowptr), ptr(src), ptr(eid), n_dst, xp, int(sr_in), ldx, xs, c, ptr(edge_attr), _ld(edge_attr), ptr(We.contiguous()),
                                      ptr(be.contiguous()), ptr(prep), ptr(a.data), ptr(a.scales), ptr(xo.data) if xo is not None else None,
                                      ptr(xo.scales) if xo is not None else None, stream_ptr())
    if rc == DGNN_E_UNSUPPORTED:
        return None
    check(rc, "dgnn_sage_aggregate_sr")
    return (a, xo) if own_rows else a


@on_device_of
def linear_sr(A1, Wp, A2=None, bias=None, scale=None, shift=None, relu=False, out_f32=False, rows=None, proj=None):
    """act(([A1 | A2] . W^T + bias) * scale + shift): A1 / A2 SplitRows, Wp = pack_rows(W1, W2, per_row=True) -> SplitRows; with out_f32 an fp32 tensor;
    with proj = (W3 [n_proj, n_out], b3 | None) the logits act(...) . W3^T + b3 [M, n_proj] (the decoder's output Linear inside the launch).
    `rows`: only the first `rows` rows of the operands.  None when the library declines the shape."""
    M = A1.size(0) if rows is None else int(rows)
    n_out = Wp.size(0)
    dev = A1.device
    c1, c2 = A1.channels, (A2.channels if A2 is not None else 0)
    if Wp.channels != c1 + c2:
        raise ValueError("packed weights have %d input channels, operands %d" % (Wp.channels, c1 + c2))
    o32 = osr = lg = W3 = b3 = None
    n_proj = 0
    if proj is not None:
        W3, b3 = proj
        W3 = _req(W3, "W3", dim=2).contiguous()
        n_proj = W3.size(0)
        if W3.size(1) != n_out or n_proj not in (1, 2):
            return None
        lg = (torch.zeros if n_out > 256 else torch.empty)((M, n_proj), dtype=torch.float32, device=dev)     # (column tiles add into zeroed logits)
    elif out_f32:
        o32 = torch.empty((M, n_out), dtype=torch.float32, device=dev)
    else:
        osr = SplitRows(torch.empty((M, n_out * 4), dtype=torch.uint8, device=dev), torch.empty((M, sr_groups(n_out)), dtype=torch.float32, device=dev), n_out)
    rc = lib().dgnn_linear_sr(ptr(A1.data), A1.data.stride(0), ptr(A1.scales), c1, ptr(A2.data) if A2 is not None else None,
                              A2.data.stride(0) if A2 is not None else 0, ptr(A2.scales) if A2 is not None else None, c2, ptr(Wp.data), ptr(Wp.scales),
                              ptr(bias), ptr(scale), ptr(shift), int(bool(relu)), M, n_out, ptr(osr.data) if osr is not None else None,
                              n_out * 4 if osr is not None else 0, ptr(osr.scales) if osr is not None else None, ptr(o32), n_out, ptr(W3), ptr(b3), n_proj, ptr(lg),
                              stream_ptr())
    if rc == DGNN_E_UNSUPPORTED:
        return None
    check(rc, "dgnn_linear_sr")
    return lg if proj is not None else (o32 if out_f32 else osr)


# ---- fused inference layer ----------------------------------------------------------------------
def fused_layer_supported(c_in: int, c_out: int, f_e: int, x: torch.Tensor = None) -> bool:
    """Mirrors the shape dispatch of dgnn_sage_layer_fused_fwd (the rule is fused::takes_f32_rows in csrc/fused_common.h): c_in <= 64 -> c_out in {64,128};
    64 < c_in <= 128 -> c_out == 128 with even c_in / row stride and 8-byte aligned rows.  Everything else takes the
    aggregate + linear pair."""
    if not FUSED_ENABLED or f_e != 20:
        return False
    if c_in <= 64:
        return c_out in (64, 128)
    if c_in <= 128:
        ok = c_out == 128 and c_in % 2 == 0
        if x is not None:
            ok = ok and x.stride(0) % 2 == 0 and x.data_ptr() % 8 == 0
        return ok
    return False


FUSED_ENABLED = True
GEMM_F32, GEMM_BF16X3, GEMM_BF16X3_FILTER, GEMM_F16X2_DENSE, GEMM_F16X2 = 0, 1, 2, 3, 4
# wide GEMMs with operands pre-split by a pass of their own and staged by DMA (dgnn_linear_fwd_x2hp, bit-identical to x2h).  OFF by default: the GEMM
# itself runs 1.3-1.5x faster (317 vs 200-260 TFLOP/s fp32-equivalent at M = 1M) but the extra write + read of the split operand costs more
# than that saves (512 -> 1024 layer 11.7 vs 10.8 ms, 256 -> 512 4.8 vs 4.2 ms; profiles/r03_wide.md)
X2HP = __import__("os").environ.get("DGNN_X2HP", "0") != "0"
GEMM_MODE_NAMES = {"f32": GEMM_F32, "bf16x3": GEMM_BF16X3, "bf16x3f": GEMM_BF16X3_FILTER, "f16x2d": GEMM_F16X2_DENSE, "f16x2": GEMM_F16X2}
# how the fused layer uses the matrix cores: exact-fp32 MFMA for the dense part ("f32"), 3-way split-bf16 MFMA for the
# dense part ("bf16x3"), or split-bf16 MFMA for the dense part AND the filter MLP ("bf16x3f"); all fp32-class accuracy
# "f16x2d" / "f16x2": the dense product (and the filter MLP) on fp16 x 2 with power-of-two group scales (22 significand bits, 3 products:
# the 3xTF32 scheme) -- half the matrix work of the bf16 x 3 forms; GEMM entry points outside the fused layer keep bf16 x 3
GEMM_MODE = GEMM_MODE_NAMES[__import__("os").environ.get("DGNN_GEMM_MODE", "f16x2")]
# whole-graph inference: fused layers read the caller's edge_attr in place (rows DMA-gathered by the plan's eid) instead of
# staging a plan-ordered copy once per scene; DGNN_EDGE_STAGING=1 restores the staged copy
EDGE_GATHER_IN_KERNEL = __import__("os").environ.get("DGNN_EDGE_STAGING", "0") != "1"


FUSED_MAX_ELEMS = 1 << 31  # row offsets inside one fused-layer launch are 32-bit element counts (tests lower it)

# optional profiling hook (bench.py): SurfaceNet._eval_layers calls tok = hook(None, c_in, c_out, n_dst, plain) right before the
# launches of one eval-mode conv layer (fused: one launch; other widths: aggregate + GEMM) and hook(tok, c_in, c_out, n_dst, plain)
# right after them, on the launching thread / current stream.  `plain`: False when the layer's launch also carries the decoder (logits
# leave it instead of rows).  While a hook is set the one-call paths step aside (SurfaceNet._one_call_tables).
LAYER_HOOK = None


def _out_rows(out, n_dst, cols, cols_name, dtype, like, out_dtypes=torch.float32):
    """result buffer of a fused layer: a fresh [n_dst, cols] tensor, or the caller's contiguous [>= n_dst, cols] one (its first n_dst rows are written)"""
    if out is None:
        return torch.empty((n_dst, cols), dtype=dtype, device=like.device)
    _req(out, "out", out_dtypes, dim=2)
    if out.size(0) < n_dst or out.size(1) != cols or out.stride(0) != cols:
        raise ValueError("out must be a contiguous [>= n_dst, %s] buffer" % cols_name)
    return out


@on_device_of
def sage_layer_fused_fwd(rowptr, src, n_dst, x_src, edge_attr, We, be, Wj, bj, Wi, scale, shift, relu, gemm_mode=None,
                         out=None, eid=None, x_dst=None, prepared=None):
    """`x_dst` (optional): own rows of the destinations when they are not x_src[:n_dst] (a destination sub-range).
    `eid` (the plan's edge ids): edge_attr is the caller's tensor in its own row order and rows are gathered inside the
    kernel; eid=None: edge_attr is already in plan order.
    `out` (optional): a [>= n_dst, c_out] buffer whose first n_dst rows receive the result (the partitioned
    forward passes the next layer's [n_own + n_halo, C] activation buffer, so no copy is needed)."""
    _req(x_src, "x_src", dim=2)
    c_in, c_out = x_src.size(1), Wj.size(0)
    out = _out_rows(out, n_dst, c_out, "c_out", torch.float32, x_src)
    mode = GEMM_MODE if gemm_mode is None else gemm_mode
    if prepared is not None and mode == GEMM_F16X2:
        # `prepared` (sage_layer_prepare): the launch skips its parameter prologue; a shape the prepared kernels do not take falls through
        rc = lib().dgnn_sage_layer_fused_fwd_p(
            ptr(rowptr), ptr(src), ptr(eid), n_dst, ptr(x_src), ptr(x_dst), _ld(x_src), c_in, ptr(edge_attr), _ld(edge_attr), We.size(1),
            ptr(We), ptr(be), ptr(Wj), ptr(bj), ptr(Wi), ptr(scale), ptr(shift), int(bool(relu)), c_out, ptr(out), c_out, ptr(prepared), stream_ptr())
        if rc != DGNN_E_UNSUPPORTED:
            check(rc, "dgnn_sage_layer_fused_fwd_p")
            return out
    check(lib().dgnn_sage_layer_fused_fwd(
        ptr(rowptr), ptr(src), ptr(eid), n_dst, ptr(x_src), ptr(x_dst), _ld(x_src), c_in, ptr(edge_attr), _ld(edge_attr), We.size(1),
        ptr(We), ptr(be), ptr(Wj), ptr(bj), ptr(Wi), ptr(scale), ptr(shift), int(bool(relu)), c_out, ptr(out), c_out,
        mode, stream_ptr()), "dgnn_sage_layer_fused_fwd")
    return out


# parameters of the fused layers prepared once per set of weights (dgnn_sage_layer_prepare); DGNN_PREPARED=0: every launch derives them itself
PREPARED_PARAMS = __import__("os").environ.get("DGNN_PREPARED", "1") != "0"


@on_device_of
def sage_layer_prepare(We, be, Wj, Wi, decoder=None):
    """-> uint8 buffer for `prepared=` of sage_layer_fused_fwd / sage_layer_fused_decoder_fwd, or None when the shape has no prepared form.
    `decoder` = (W0, b0, scale1, shift1, W3, b3) for the last layer's launch that carries the decoder."""
    c_in, c_out = Wj.size(1), Wj.size(0)
    nbytes = int(lib().dgnn_sage_layer_prepared_bytes(c_in, c_out, int(decoder is not None)))
    if nbytes <= 0 or We.size(1) != 20:
        return None
    buf = torch.empty(nbytes, dtype=torch.uint8, device=Wj.device)
    d = decoder if decoder is not None else (None,) * 6
    rc = lib().dgnn_sage_layer_prepare(c_in, c_out, ptr(We.contiguous()), ptr(be), ptr(Wj.contiguous()), ptr(Wi.contiguous()),
                                       ptr(d[0].contiguous() if d[0] is not None else None), ptr(d[1]), ptr(d[2]), ptr(d[3]),
                                       ptr(d[4].contiguous() if d[4] is not None else None), ptr(d[5]), ptr(buf), stream_ptr())
    if rc == DGNN_E_UNSUPPORTED:
        return None
    check(rc, "dgnn_sage_layer_prepare")
    return buf


# the last conv layer and the decoder in one launch (dgnn_sage_layer_fused_decoder_fwd); DGNN_FUSE_DECODER=0 keeps them apart
FUSE_DECODER = __import__("os").environ.get("DGNN_FUSE_DECODER", "1") != "0"


def fused_layer_decoder_supported(c_in: int, c_out: int, f_e: int, hidden: int, n_out: int, x=None) -> bool:
    """shipped shape only: 64 < c_in <= 128, c_out 128, 20 edge attributes, decoder 128 -> 64 -> 2, default arithmetic, fp32 rows"""
    ok = (FUSE_DECODER and FUSED_ENABLED and GEMM_MODE == GEMM_F16X2 and 64 < c_in <= 128 and c_in % 8 == 0 and c_out == 128 and f_e == 20
          and hidden == 64 and n_out == 2)
    if ok and x is not None:
        ok = x.dtype == torch.float32 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
    return ok


@on_device_of
def sage_layer_fused_decoder_fwd(rowptr, src, n_dst, x_src, edge_attr, We, be, Wj, bj, Wi, scale, shift, relu, W0, b0, scale1, shift1, W3, b3,
                                 out=None, eid=None, x_dst=None, prepared=None):
    """Last conv layer + decoder, one launch -> logits [n_dst, 2] (written into `out` when given: a contiguous [>= n_dst, 2] fp32 buffer)."""
    _req(x_src, "x_src", dim=2)
    out = _out_rows(out, n_dst, 2, "2", torch.float32, x_src)
    head = (ptr(rowptr), ptr(src), ptr(eid), n_dst, ptr(x_src), ptr(x_dst), _ld(x_src), x_src.size(1), ptr(edge_attr), _ld(edge_attr), We.size(1),
            ptr(We), ptr(be), ptr(Wj), ptr(bj), ptr(Wi), ptr(scale), ptr(shift), int(bool(relu)), Wj.size(0), ptr(W0.contiguous()), ptr(b0),
            ptr(scale1), ptr(shift1), W0.size(0), ptr(W3.contiguous()), ptr(b3), W3.size(0), ptr(out))
    if prepared is not None:
        check(lib().dgnn_sage_layer_fused_decoder_fwd_p(*head, ptr(prepared), stream_ptr()), "dgnn_sage_layer_fused_decoder_fwd_p")
    else:
        check(lib().dgnn_sage_layer_fused_decoder_fwd(*head, stream_ptr()), "dgnn_sage_layer_fused_decoder_fwd")
    return out


# whole-scene inference as ONE library call (dgnn_static_infer_fwd: plan + every conv layer + decoder); DGNN_INFER_ONE_CALL=0 keeps the per-layer calls
INFER_ONE_CALL = __import__("os").environ.get("DGNN_INFER_ONE_CALL", "1") != "0"


def _infer_tables(x_width, layers, decoder, prepared, cache):
    """ctypes argument tables of the one-call entry points: (L, widths, 7 per-layer pointer arrays, prepared, the decoder's 8 scalars / addresses,
    n_out); kept in `cache` (the model's, valid as long as the tensors are: SurfaceNet._one_call_tables) when one is given."""
    if cache is not None:
        hit = cache.get(x_width)
        if hit is not None:
            return hit
    L = len(layers)
    widths = [x_width] + [l[2].size(0) for l in layers]
    w_arr = (C.c_int32 * (L + 1))(*widths)
    cols = tuple((C.c_void_p * L)(*[(l[i].data_ptr() if l[i] is not None else None) for l in layers]) for i in range(7))
    prep = (C.c_void_p * L)(*[(p.data_ptr() if p is not None else None) for p in prepared]) if prepared is not None else None
    d = decoder if decoder is not None else (None,) * 6
    dec = (ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), d[0].size(0) if d[0] is not None else 0, ptr(d[4]), ptr(d[5]), d[4].size(0) if d[4] is not None else 0)
    out = (L, w_arr, cols, prep, dec, decoder[4].size(0) if decoder is not None else widths[-1])
    if cache is not None:
        cache[x_width] = out
    return out


def _one_call(name, x, edge_attr, edge_index, plan_parts, hint, n_key, n_work, n_rows, mid, tables, tail):
    """The body the one-call family shares (dgnn_static_infer_*; call under on_device_of): plan arrays of the first `n_key` cells (allocated and built
    inside the call unless `plan_parts` brings them), logits [n_rows, n_out] and the workspace of `n_work` rows; the library call gets the edge_index
    triple, the plan, `mid` (what the entry point takes between the plan and x), the rows, the tables and `tail` (what it takes between the tables and
    the workspace).  -> (logits, plan parts), or None when the library refuses the configuration (nothing launched)."""
    _req(x, "x", dim=2)
    _req(edge_attr, "edge_attr", dim=2)
    dev = x.device
    L, w_arr, cols, _, _, n_out = tables
    E = edge_index.size(1) if edge_index is not None else plan_parts[1].numel()
    build = plan_parts is None
    if build:
        rowptr = torch.empty(n_key + 1, dtype=torch.int32, device=dev)
        src = torch.empty(max(E, 1), dtype=torch.int32, device=dev)[:E]
        eid = torch.empty(max(E, 1), dtype=torch.int32, device=dev)[:E]
        scratch = torch.empty(int(lib().dgnn_plan_scratch_elems(E, n_key)), dtype=torch.int32, device=dev)
        plan_parts = (rowptr, src, eid)
    else:
        rowptr, src, eid = plan_parts
        scratch = None
    logits = torch.empty((n_rows, n_out), dtype=torch.float32, device=dev)
    work = torch.empty(int(lib().dgnn_static_infer_workspace_bytes(n_work, L, w_arr)), dtype=torch.uint8, device=dev)   # (the caching allocator hands out 512-byte aligned blocks)
    rc = getattr(lib(), name)(
        ptr(edge_index) if build else None, edge_index.stride(0) if build else 0, edge_index.stride(1) if build else 0, E, hint, ptr(rowptr), ptr(src),
        ptr(eid), ptr(scratch), *mid, ptr(x), _ld(x), ptr(edge_attr), _ld(edge_attr), edge_attr.size(1), L, w_arr, *cols, *tail, ptr(work), ptr(logits),
        stream_ptr())
    if rc == DGNN_E_UNSUPPORTED:
        return None
    check(rc, name, poll=build)
    return logits, plan_parts


def _n_dst_array(n_dst, L):
    assert len(n_dst) == L
    return (C.c_int64 * L)(*[int(v) for v in n_dst])


@on_device_of
def static_infer_fwd(x, edge_attr, edge_index, plan_parts, layers, decoder, prepared=None, hint=PLAN_HINT_REFERENCE, gemm_mode=None, fuse_decoder=True, cache=None):
    """-> (logits | last activations, plan parts) or None when a shape is outside the fused kernels (nothing launched).
    `plan_parts` = (rowptr, src, eid) of an existing plan, or None: the plan is built inside the call from `edge_index` (int64 [2,E], any strides)
    and its arrays are returned.  `layers`: per conv layer (We, be, Wj, bj, Wi, scale | None, shift | None); `decoder` = (W0, b0, scale1 | None,
    shift1 | None, W3, b3) or None; `prepared`: per-layer dgnn_sage_layer_prepare buffers or None; `fuse_decoder`: the last layer's launch carries the
    decoder (prepared[-1] is then the block made WITH the decoder), else layer and decoder run apart.  `cache`: see _infer_tables."""
    t = _infer_tables(x.size(1), layers, decoder, prepared, cache)
    n = x.size(0)
    return _one_call("dgnn_static_infer_fwd", x, edge_attr, edge_index, plan_parts, hint, n, n, n, (n,), t,
                     (t[3], *t[4], int(bool(fuse_decoder)), GEMM_MODE if gemm_mode is None else gemm_mode))


@on_device_of
def static_infer_rings_fwd(x, edge_attr, edge_index, plan_parts, n_dst, layers, decoder, prepared=None, hint=PLAN_HINT_GROUPED, gemm_mode=None, fuse_decoder=True,
                           attr_in_plan_order=True, cache=None):
    """One rank's part of a partitioned scene, rings of halo cells recomputed instead of exchanged (dgnn_static_infer_rings_fwd; arguments as
    static_infer_fwd): x [n_loc, F] local rows (owned cells, ring 1, ring 2, ...), `edge_index` the local list (in-edges of the first n_dst[0] cells),
    n_dst[l] = destinations of layer l.  -> (logits [n_dst[-1], n_logits], plan parts) or None (nothing launched)."""
    t = _infer_tables(x.size(1), layers, decoder, prepared, cache)
    return _one_call("dgnn_static_infer_rings_fwd", x, edge_attr, edge_index, plan_parts, hint, n_dst[0], n_dst[0], n_dst[-1],
                     (int(bool(attr_in_plan_order)), x.size(0), _n_dst_array(n_dst, t[0])), t,
                     (t[3], *t[4], int(bool(fuse_decoder)), GEMM_MODE if gemm_mode is None else gemm_mode))


@on_device_of
def static_infer_rings_fwd_bf16(x, edge_attr, edge_index, plan_parts, n_dst, layers, decoder, hint=PLAN_HINT_GROUPED, attr_in_plan_order=True, cache=None):
    """static_infer_rings_fwd in bf16 STORAGE (dgnn_static_infer_rings_fwd_bf16): fp32 input rows read in place by the first layer, 16-bit rows (unsigned
    with BF16_UNSIGNED_ROWS) between the layers, the decoder inside the last launch.  A whole scene is n_dst = [n] * L.  None: nothing launched."""
    assert decoder is not None
    t = _infer_tables(x.size(1), layers, decoder, None, cache)
    return _one_call("dgnn_static_infer_rings_fwd_bf16", x, edge_attr, edge_index, plan_parts, hint, n_dst[0], n_dst[0], n_dst[-1],
                     (int(bool(attr_in_plan_order)), x.size(0), _n_dst_array(n_dst, t[0])), t,
                     (*t[4], BF16_MODE | (BF16_ROWS_OUT_UNSIGNED if BF16_UNSIGNED_ROWS else 0)))


@on_device_of
def static_infer_partitioned_fwd(x, edge_attr, edge_index, plan_parts, n_own, n_interior, layers, decoder, prepared=None, halo=None, comm=None, send_buf=None,
                                 hint=PLAN_HINT_GROUPED, gemm_mode=None, fuse_decoder=True, attr_in_plan_order=True, cache=None):
    """One rank's part of a partitioned scene in one library call (dgnn_static_infer_partitioned_fwd; arguments as static_infer_fwd): x [n_own + n_halo, F]
    local rows, `edge_index` the local list (destinations < n_own), `halo` / `comm` the library's halo plan and communicator (None: a single-rank
    part), `send_buf` a uint8 buffer of n_send * max hidden width * 4 bytes.  -> (logits [n_own, n_logits], plan parts) or None (nothing launched)."""
    t = _infer_tables(x.size(1), layers, decoder, prepared, cache)
    return _one_call("dgnn_static_infer_partitioned_fwd", x, edge_attr, edge_index, plan_parts, hint, n_own, x.size(0), n_own,
                     (int(bool(attr_in_plan_order)), n_own, n_interior, x.size(0) - n_own), t,
                     (t[3], *t[4], int(bool(fuse_decoder)), GEMM_MODE if gemm_mode is None else gemm_mode, halo, comm, ptr(send_buf)))


def decoder_fused_supported(k: int, hidden: int, n_out: int) -> bool:
    return k == 128 and hidden == 64 and n_out in (1, 2)


@on_device_of
def decoder_fused_fwd(y, W0, b0, scale, shift, W3, b3):
    _req(y, "y", dim=2)
    M, n_out = y.size(0), W3.size(0)
    out = torch.empty((M, n_out), dtype=torch.float32, device=y.device)
    check(lib().dgnn_decoder_fused_fwd(ptr(y), _ld(y), M, y.size(1), ptr(W0.contiguous()), ptr(b0), ptr(scale), ptr(shift),
                                       W0.size(0), ptr(W3.contiguous()), ptr(b3), n_out, ptr(out), n_out, stream_ptr()),
          "dgnn_decoder_fused_fwd")
    return out


# ---- bf16 storage path (BASELINE config 3) ----------------------------------------------------------------------------------
BF16 = torch.bfloat16
# UNSIGNED rows (round 4; include/dgnn_hip.h DGNN_BF16_ROWS_*_UNSIGNED): rows written behind a ReLU keep the fp32 bits [30:15] -- 8 exponent + 8 mantissa
# bits, no sign -- in their 16 bits: half the storage rounding of bf16 in the same bytes.  Such rows travel in torch.int16 tensors (the dtype IS the
# format: it survives slicing, cat and the halo exchange), written and read by the fused bf16-storage layers only; rows_unsigned_to_bf16 converts for
# every other consumer.  DGNN_BF16_UNSIGNED_ROWS=0: plain bf16 rows everywhere (rounds 2-3).
UROWS = torch.int16
BF16_UNSIGNED_ROWS = __import__("os").environ.get("DGNN_BF16_UNSIGNED_ROWS", "1") != "0"
BF16_ROWS_IN_UNSIGNED, BF16_ROWS_OUT_UNSIGNED = 16, 32
BF16_SINGLE, BF16_COMPENSATED = 0, 1
# how the fused bf16-storage kernels feed the matrix cores: "single" = every operand rounded to bf16 once; "compensated"
# (default) = only the stored activations are bf16, the fp32 mean / attributes / parameters go in as (hi, lo) bf16 pairs
BF16_MODE = {"single": BF16_SINGLE, "compensated": BF16_COMPENSATED}[__import__("os").environ.get("DGNN_BF16_MODE", "compensated")]


@on_device_of
def cast_to_bf16(x: torch.Tensor, cols_pad: int = None) -> torch.Tensor:
    """fp32 [n, cols] (any row stride) -> bf16 [n, cols_pad] with zero padding columns (cols_pad even, default: cols rounded up to even)."""
    _req(x, "x", dim=2)
    n, cols = x.shape
    if cols_pad is None:
        cols_pad = (cols + 1) // 2 * 2
    out = torch.empty((n, cols_pad), dtype=BF16, device=x.device)
    check(lib().dgnn_cast_f32_to_bf16(ptr(x), _ld(x), n, cols, cols_pad, ptr(out), cols_pad, stream_ptr()), "dgnn_cast_f32_to_bf16")
    return out


@on_device_of
def rows_unsigned_to_bf16(x: torch.Tensor) -> torch.Tensor:
    """unsigned rows (int16 container) -> plain bf16 rows, round to nearest even"""
    _req(x, "x", UROWS, dim=2)
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    check(lib().dgnn_rows_unsigned_to_bf16(ptr(x), _ld(x), x.size(0), x.size(1), ptr(out), x.size(1), stream_ptr()), "dgnn_rows_unsigned_to_bf16")
    return out


@on_device_of
def cast_to_f32(x: torch.Tensor) -> torch.Tensor:
    if x.dtype == UROWS:
        x = rows_unsigned_to_bf16(x)
    _req(x, "x", BF16, dim=2)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib().dgnn_cast_bf16_to_f32(ptr(x), _ld(x), x.size(0), x.size(1), ptr(out), x.size(1), stream_ptr()), "dgnn_cast_bf16_to_f32")
    return out


def fused_layer_supported_bf16(c_in: int, c_out: int, f_e: int, x: torch.Tensor = None) -> bool:
    """Mirrors the shape dispatch of dgnn_sage_layer_fused_fwd_bf16 (the rule is fused::takes_bf16_rows in csrc/fused_common.h).  `x` fp32: the first layer reading the
    caller's fp32 features in place (c_in <= 32)."""
    if not FUSED_ENABLED or f_e != 20 or c_in > 128 or c_out not in (64, 128):
        return False
    nb = 2 if c_in <= 32 else (4 if c_in <= 64 else 8)
    ok = c_in % nb == 0
    if x is not None and x.dtype == torch.float32:
        return ok and c_in <= 32 and x.data_ptr() % 4 == 0
    if x is not None:
        ok = ok and x.stride(0) % nb == 0 and x.data_ptr() % (2 * nb) == 0
    return ok


@on_device_of
def sage_layer_fused_fwd_bf16(rowptr, src, n_dst, x_src, c_in, edge_attr, We, be, Wj, bj, Wi, scale, shift, relu, out=None, eid=None,
                              x_dst=None, rows_out_unsigned=False):
    """bf16-storage twin of sage_layer_fused_fwd.  `x_src` bf16 [n_src, ld >= c_in] (padding columns allowed: `c_in` is the
    logical width = Wj.shape[1]) -- or, for the first layer (c_in <= 32), the caller's fp32 rows read in place; returns bf16
    [n_dst, c_out]."""
    _req(x_src, "x_src", ACT + (UROWS,), dim=2)
    _same(x_dst, x_src, "x_dst")
    c_out = Wj.size(0)
    out = _out_rows(out, n_dst, c_out, "c_out", UROWS if rows_out_unsigned else BF16, x_src, (BF16, UROWS))      # a given buffer's dtype names the row format it receives
    fmt = (BF16_ROWS_IN_UNSIGNED if x_src.dtype == UROWS else 0) | (BF16_ROWS_OUT_UNSIGNED if out.dtype == UROWS else 0)
    check(lib().dgnn_sage_layer_fused_fwd_bf16(
        ptr(rowptr), ptr(src), ptr(eid), n_dst, ptr(x_src), int(x_src.dtype == torch.float32), ptr(x_dst), _ld(x_src), c_in, ptr(edge_attr),
        _ld(edge_attr), We.size(1),
        ptr(We), ptr(be), ptr(Wj), ptr(bj), ptr(Wi), ptr(scale), ptr(shift), int(bool(relu)), c_out, ptr(out), c_out, BF16_MODE | fmt, stream_ptr()),
        "dgnn_sage_layer_fused_fwd_bf16")
    return out


def fused_layer_decoder_supported_bf16(c_in: int, c_out: int, f_e: int, hidden: int, n_out: int, x=None) -> bool:
    """the last bf16-storage layer's launch can carry the decoder: shipped shape, compensated arithmetic, bf16 rows 16-byte aligned"""
    ok = (FUSE_DECODER and FUSED_ENABLED and BF16_MODE == BF16_COMPENSATED and 64 < c_in <= 128 and c_in % 8 == 0 and c_out == 128 and f_e == 20
          and hidden == 64 and n_out == 2)
    if ok and x is not None:
        ok = x.dtype in (torch.bfloat16, UROWS) and x.stride(1) == 1 and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0
    return ok


@on_device_of
def sage_layer_fused_decoder_fwd_bf16(rowptr, src, n_dst, x_src, c_in, edge_attr, We, be, Wj, bj, Wi, scale, shift, relu, W0, b0, scale1, shift1, W3, b3,
                                      out=None, eid=None, x_dst=None):
    """Last conv layer (bf16 storage) + decoder, one launch -> fp32 logits [n_dst, 2]; the layer's output is never rounded to bf16."""
    _req(x_src, "x_src", (BF16, UROWS), dim=2)
    _same(x_dst, x_src, "x_dst")
    out = _out_rows(out, n_dst, 2, "2", torch.float32, x_src)
    check(lib().dgnn_sage_layer_fused_decoder_fwd_bf16(
        ptr(rowptr), ptr(src), ptr(eid), n_dst, ptr(x_src), ptr(x_dst), _ld(x_src), c_in, ptr(edge_attr), _ld(edge_attr), We.size(1), ptr(We), ptr(be),
        ptr(Wj), ptr(bj), ptr(Wi), ptr(scale), ptr(shift), int(bool(relu)), Wj.size(0), ptr(W0.contiguous()), ptr(b0), ptr(scale1), ptr(shift1), W0.size(0),
        ptr(W3.contiguous()), ptr(b3), W3.size(0), ptr(out), BF16_MODE | (BF16_ROWS_IN_UNSIGNED if x_src.dtype == UROWS else 0), stream_ptr()),
        "dgnn_sage_layer_fused_decoder_fwd_bf16")
    return out


@on_device_of
def decoder_fused_fwd_bf16(y, W0, b0, scale, shift, W3, b3):
    _req(y, "y", BF16, dim=2)
    M, n_out = y.size(0), W3.size(0)
    out = torch.empty((M, n_out), dtype=torch.float32, device=y.device)
    check(lib().dgnn_decoder_fused_fwd_bf16(ptr(y), _ld(y), M, y.size(1), ptr(W0.contiguous()), ptr(b0), ptr(scale), ptr(shift),
                                            W0.size(0), ptr(W3.contiguous()), ptr(b3), n_out, ptr(out), n_out, BF16_MODE, stream_ptr()),
          "dgnn_decoder_fused_fwd_bf16")
    return out


# ---- training-mode conv layer, one call each way (csrc/train.hip) -----------------------------------------------------------
TRAIN_COMPOSITE = __import__("os").environ.get("DGNN_TRAIN_COMPOSITE", "1") != "0"
TRAIN_WHOLE_MODEL = __import__("os").environ.get("DGNN_TRAIN_WHOLE_MODEL", "1") != "0"   # Static fp32: all layers in one call each way
TRAIN_DECODER_OUTPUT_IN_CALL = __import__("os").environ.get("DGNN_TRAIN_DECODER_IN_CALL", "1") != "0"   # ... the decoder's output Linear too
# the direct training step keeps ONE gradient buffer per model and rewrites it in place (p.grad stays the same tensor from step to step, as after
# zero_grad(set_to_none=False)); 0 = fresh gradient tensors every step
TRAIN_KEEP_GRADS = __import__("os").environ.get("DGNN_TRAIN_KEEP_GRADS", "1") != "0"


def _grad_buffer(rows, dev):
    """The parameter gradients of a backward call as views of ONE fp32 buffer.  `rows`: per layer the gradients' shapes, (r, c) | (n,), None or an
    empty shape where the layer has no such parameter.  -> (flat, offs, views): element offsets and views per layer in the order of `rows`, None
    where there is no gradient.  One allocation and one view op per gradient (a slice + .view pair costs 2.5 x as much on the host)."""
    offs, off = [], 0
    for row in rows:
        o = []
        for sh in row:
            n = 0 if sh is None else sh[0] * sh[1] if len(sh) == 2 else sh[0]
            o.append(off if n else None)
            off += n
        offs.append(o)
    flat = torch.empty(off, dtype=torch.float32, device=dev)
    st = torch.as_strided
    views = [tuple(None if o is None else st(flat, sh, (sh[1], 1) if len(sh) == 2 else (1,), o) for sh, o in zip(row, oo)) for row, oo in zip(rows, offs)]
    return flat, offs, views


@on_device_of
def sage_layer_train_fwd(plan_parts, n_dst, x, edge_attr, We, be, Wj, bj, Wi, gamma, beta, running_mean, running_var, momentum, eps, relu):
    """conv (aggregate + lin_j + lin_i) -> BatchNorm(batch statistics, running buffers updated) -> ReLU as ONE library call; fp32 or
    bf16 storage (the type of x).  `plan_parts` = (rowptr, src, eid) of the destination-sorted plan, or None for a plain
    Linear + BatchNorm block (decoder).  -> (y, a | None, z, stats[4, c_out] = mean, var, scale, shift)"""
    _req(x, "x", ACT, dim=2)
    c_in, c_out = x.size(1), Wj.size(0)
    dev, dt = x.device, x.dtype
    rowptr = src = eid = a = None
    f_e = 0
    if plan_parts is not None:
        rowptr, src, eid = plan_parts
        a = torch.empty((n_dst, c_in), dtype=dt, device=dev)
        if We is not None:
            _req(edge_attr, "edge_attr", dim=2)
            f_e = We.size(1)
            if We.size(0) != c_in or edge_attr.size(1) < f_e:
                raise ValueError("lin_e weight %s does not match c_in=%d / edge_attr %s" % (tuple(We.shape), c_in, tuple(edge_attr.shape)))
    if Wj.size(1) != c_in or (Wi is not None and tuple(Wi.shape) != tuple(Wj.shape)):
        raise ValueError("lin_j / lin_i weights do not match c_in=%d" % c_in)
    z = torch.empty((n_dst, c_out), dtype=dt, device=dev)
    y = torch.empty((n_dst, c_out), dtype=dt, device=dev)
    stats = torch.empty((4, c_out), dtype=torch.float32, device=dev)
    scratch = _f32(lib().dgnn_colstats_scratch_elems(n_dst, c_out), dev)
    head = (ptr(rowptr), ptr(src), ptr(eid), n_dst, ptr(x), _ld(x), c_in, ptr(edge_attr) if f_e else None, _ld(edge_attr) if f_e else 0, f_e,
            ptr(We), ptr(be), ptr(Wj), ptr(bj), ptr(Wi), c_out, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), float(momentum), float(eps),
            int(bool(relu)), ptr(a), ptr(z), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), ptr(y), ptr(scratch))
    if dt == torch.bfloat16:
        check(lib().dgnn_sage_layer_train_fwd_bf16(*head, stream_ptr()), "dgnn_sage_layer_train_fwd_bf16")
    else:
        check(lib().dgnn_sage_layer_train_fwd(*head, GEMM_MODE, stream_ptr()), "dgnn_sage_layer_train_fwd")
    _written_behind_torch(running_mean, running_var)
    return y, a, z, stats


@on_device_of
def sage_layer_train_bwd(t_parts, rowptr_dst, n_src, n_dst, x, edge_attr, We, be, Wj, Wi, has_bias, gamma, stats, eps, relu, a, z, y, dy, need_dx):
    """backward of sage_layer_train_fwd as ONE library call -> (dx | None, dWe, dbe, dWj, dbj, dWi, dgamma, dbeta); parameter
    gradients are fp32 views of one buffer, dx has the storage type of x."""
    c_in, c_out = x.size(1), Wj.size(0)
    dev, dt = x.device, x.dtype
    agg = t_parts is not None
    f_e = We.size(1) if (agg and We is not None) else 0
    _, _, ((dWe, dbe, dWj, dbj, dWi, dgamma, dbeta),) = _grad_buffer([[(c_in, f_e), (c_in,) if f_e else None, (c_out, c_in), (c_out,) if has_bias else None,
                                                                       (c_out, c_in) if (agg and Wi is not None) else None, (c_out,), (c_out,)]], dev)
    dx = torch.empty((n_src if agg else n_dst, c_in), dtype=dt, device=dev) if need_dx else None
    scratch = _f32(lib().dgnn_sage_layer_train_scratch_elems(n_src, n_dst, c_in, c_out, f_e), dev)
    t_rowptr, t_dst, t_eid = t_parts if agg else (None, None, None)
    head = (ptr(t_rowptr), ptr(t_dst), ptr(t_eid), ptr(rowptr_dst), n_src, n_dst, ptr(x), _ld(x), c_in, ptr(edge_attr) if f_e else None,
            _ld(edge_attr) if f_e else 0, f_e, ptr(We), ptr(be), ptr(Wj), ptr(Wi), c_out, ptr(gamma), ptr(stats[0]), ptr(stats[1]), float(eps),
            int(bool(relu)), ptr(a), ptr(z), ptr(y), ptr(dy), ptr(dx), ptr(dWe), ptr(dbe), ptr(dWj), ptr(dbj), ptr(dWi), ptr(dgamma), ptr(dbeta))
    if dt == torch.bfloat16:
        dz = torch.empty((n_dst, c_out), dtype=dt, device=dev)
        da = torch.empty((n_dst, c_in), dtype=dt, device=dev) if agg else None
        check(lib().dgnn_sage_layer_train_bwd_bf16(*head, ptr(dz), ptr(da), ptr(scratch), stream_ptr()), "dgnn_sage_layer_train_bwd_bf16")
    else:
        check(lib().dgnn_sage_layer_train_bwd(*head, ptr(scratch), GEMM_MODE, stream_ptr()), "dgnn_sage_layer_train_bwd")
    return (dx, dWe, dbe, dWj, dbj, dWi, dgamma, dbeta)


# ---- all conv layers of the Updated variant per call (csrc/train.hip: dgnn_updated_stack_fwd / _bwd) ---------------------------------------
UPDATED_STACK = __import__("os").environ.get("DGNN_UPDATED_STACK", "1") != "0"
_UPDATED_ARRAYS = {}
UPDATED_TAIL_IN_CALL = __import__("os").environ.get("DGNN_UPDATED_TAIL_IN_CALL", "1") != "0"   # ... and the model's output network behind it


@on_device_of
def updated_stack_fwd(x0, edge_attr_all, pos, layers):
    """`layers`: per conv layer a dict with plan (GraphPlan), e_id (int64 [E_l], rows of the scene's edge tensor), rows0 (int32 form of e_id, layer 0),
    edge_in, relu, We, be, Wl, bl, Wr.  -> (y_last, saved): every layer's ea / phi / a / y (+ the chaining's inverse maps) in one buffer."""
    _req(x0, "x", ACT, dim=2)
    _req(edge_attr_all, "edge_attr", dim=2)
    dev, dt, L = x0.device, x0.dtype, len(layers)
    bf = dt == torch.bfloat16
    widths = [x0.size(1)] + [l["Wl"].size(0) for l in layers]
    esz = 2 if bf else 4
    offs, off = [], 0          # byte offsets into one buffer, every piece 16-byte aligned

    def take(nbytes):
        nonlocal off
        o = off
        off += (nbytes + 15) & ~15
        return o
    for i, l in enumerate(layers):
        p = l["plan"]
        E, n, ci, co, k = p.E, p.n_dst, widths[i], widths[i + 1], l["edge_in"]
        if l["Wl"].size(1) != ci or l["We"].size(0) != ci or l["We"].size(1) != k:
            raise ValueError("Updated conv %d: lin_e %s / lin_l %s do not match %d input channels, %d edge columns" % (i, tuple(l["We"].shape), tuple(l["Wl"].shape), ci, k))
        ld_ea = (k + 1) // 2 * 2 if (bf and i == 0) else k
        offs.append(dict(ea=take(max(E, 1) * ld_ea * esz), ld_ea=ld_ea, phi=take(max(E, 1) * ci * esz), a=take(n * ci * esz), y=take(n * co * esz),
                         inv=take(4 * max(layers[i - 1]["plan"].E, 1)) if i else None))
    ea0 = take(4 * max(layers[0]["plan"].E, 1) * layers[0]["edge_in"]) if bf else None
    buf = torch.empty(off, dtype=torch.uint8, device=dev)
    base = buf.data_ptr()
    at = lambda o: None if o is None else base + o
    parts = [l["plan"].part_ptrs(False) for l in layers]
    arr = lambda k: _parr([l[k] for l in layers])
    i64 = lambda v: _iarr(v, C.c_int64)
    i32 = lambda v: _iarr(v, C.c_int32)
    # tables of what belongs to the MODEL (parameter addresses, widths, edge_in, relu flags): rebuilt only when an address has moved
    names = ("We", "be", "Wl", "bl", "Wr")
    key = tuple((l[k].data_ptr() if l[k] is not None else 0) for l in layers for k in names) + tuple((l["edge_in"], bool(l["relu"])) for l in layers) + (x0.size(1),)
    hit = _UPDATED_ARRAYS.get(L)
    if hit is None or hit[0] != key:
        hit = (key, dict({k: arr(k) for k in names}, widths=i32(widths), edge_in=i32([l["edge_in"] for l in layers]),
                         relu=i32([int(bool(l["relu"])) for l in layers])))
        _UPDATED_ARRAYS[L] = hit
    pa = hit[1]
    check(lib().dgnn_updated_stack_fwd(
        L, _parr([p[0] for p in parts]), _parr([p[1] for p in parts]), _parr([p[2] for p in parts]), arr("e_id"), ptr(layers[0]["rows0"]),
        i64([l["plan"].n_dst for l in layers]), i64([l["plan"].E for l in layers]), ptr(x0), _ld(x0), pa["widths"], pa["edge_in"],
        ptr(edge_attr_all), _ld(edge_attr_all), edge_attr_all.size(0), ptr(pos), pa["We"], pa["be"], pa["Wl"], pa["bl"], pa["Wr"],
        pa["relu"], _parr([at(o["ea"]) for o in offs]), i64([o["ld_ea"] for o in offs]), at(ea0),
        _parr([at(o["phi"]) for o in offs]), _parr([at(o["a"]) for o in offs]), _parr([at(o["y"]) for o in offs]), _parr([at(o["inv"]) for o in offs]),
        int(bf), GEMM_MODE, stream_ptr()), "dgnn_updated_stack_fwd", poll=True)
    n, co = layers[-1]["plan"].n_dst, widths[-1]
    y = torch.as_strided(buf.view(dt), (n, co), (co, 1), offs[-1]["y"] // esz)
    return y, (buf, offs, widths, pa)


@on_device_of
def updated_stack_bwd(x0, layers, saved, dy):
    """-> per layer (dWe, dbe, dWl, dbl | None, dWr | None): views of one fp32 buffer"""
    buf, offs, widths, pa = saved
    dev, dt, L = x0.device, x0.dtype, len(layers)
    bf = dt == torch.bfloat16
    base = buf.data_ptr()
    at = lambda o: None if o is None else base + o
    flat, goffs, grads = _grad_buffer([[(widths[i], l["edge_in"]), (widths[i],), (widths[i + 1], widths[i]), (widths[i + 1],) if l["bl"] is not None else None,
                                        (widths[i + 1], widths[i]) if l["Wr"] is not None else None] for i, l in enumerate(layers)], dev)
    gbase = flat.data_ptr()
    gat = lambda o: None if o is None else gbase + 4 * o
    P = [l["plan"] for l in layers]
    mx = lambda vals: max(list(vals) + [1])
    # the seven work buffers of the backward (storage type) as pieces of one allocation, 16-byte aligned
    esz = 2 if bf else 4
    counts = [mx(P[i].n_src * widths[i] for i in range(1, L)) if L > 1 else 0] * 2 + [
        mx(P[i].E * layers[i]["edge_in"] for i in range(1, L)) if L > 1 else 0, mx(P[i].E * widths[i] for i in range(L - 1)) if L > 1 else 0,
        mx(P[i].n_dst * widths[i + 1] for i in range(L)), mx(2 * P[i].n_dst * widths[i] for i in range(L)), mx(P[i].E * widths[i] for i in range(L))]
    woffs, wtot = [], 0
    for c in counts:
        woffs.append(wtot)
        wtot += (c * esz + 15) & ~15
    wbuf = torch.empty(max(wtot, 16), dtype=torch.uint8, device=dev)
    wbase = wbuf.data_ptr()
    wptr = [(wbase + o) if c else None for o, c in zip(woffs, counts)]
    dxb, d_ea, dphi_ext, dz, da, dphi = wptr[0:2], wptr[2], wptr[3], wptr[4], wptr[5], wptr[6]
    scratch = _f32(max(lib().dgnn_sage_updated_train_scratch_elems(P[i].n_dst, P[i].E, widths[i], widths[i + 1], layers[i]["edge_in"]) for i in range(L)), dev)
    tps = [p.transposed_ptrs(False) for p in P]
    arr = lambda k: _parr([l[k] for l in layers])
    i64 = lambda v: _iarr(v, C.c_int64)
    i32 = lambda v: _iarr(v, C.c_int32)
    col = lambda j: _parr([gat(r[j]) for r in goffs])
    check(lib().dgnn_updated_stack_bwd(
        L, _parr([t[0] for t in tps]), _parr([t[1] for t in tps]), _parr([t[2] for t in tps]), _parr([p.part_ptrs(False)[0] for p in P]),
        i64([p.n_src for p in P]), i64([p.n_dst for p in P]), i64([p.E for p in P]), ptr(x0), _ld(x0), pa["widths"], pa["edge_in"],
        pa["We"], pa["Wl"], pa["Wr"], pa["relu"], _parr([at(o["ea"]) for o in offs]), i64([o["ld_ea"] for o in offs]),
        _parr([at(o["phi"]) for o in offs]), _parr([at(o["a"]) for o in offs]), _parr([at(o["y"]) for o in offs]), _parr([at(o["inv"]) for o in offs]),
        ptr(dy), col(0), col(1), col(2), col(3), col(4), _parr(dxb), d_ea, dphi_ext, dz, da, dphi, ptr(scratch), int(bf), GEMM_MODE,
        stream_ptr()), "dgnn_updated_stack_bwd")
    return grads


@on_device_of
def updated_tail_fwd(x, W1, b1, W3, b3):
    """out_net behind the conv stack: -> (logits fp32 [n, n_out], h [n, hdim] in x's type)"""
    n, c, hd, no = x.size(0), x.size(1), W1.size(0), W3.size(0)
    h = torch.empty((n, hd), dtype=x.dtype, device=x.device)
    logits = torch.empty((n, no), dtype=torch.float32, device=x.device)
    check(lib().dgnn_updated_tail_fwd(n, ptr(x), _ld(x), c, ptr(W1), ptr(b1), hd, ptr(W3), ptr(b3), no, ptr(h), ptr(logits), int(x.dtype == torch.bfloat16),
                                      GEMM_MODE, stream_ptr()), "dgnn_updated_tail_fwd")
    return logits, h


@on_device_of
def updated_tail_bwd(x, W1, W3, h, g):
    """-> (dx [n, c] in x's type, dW1, db1, dW3, db3)"""
    n, c, hd, no = x.size(0), x.size(1), W1.size(0), W3.size(0)
    _, _, ((dW1, db1, dW3, db3),) = _grad_buffer([[(hd, c), (hd,), (no, hd), (no,)]], x.device)
    dx = torch.empty((n, c), dtype=x.dtype, device=x.device)
    dh = torch.empty((n, hd), dtype=x.dtype, device=x.device)
    scratch = _f32(lib().dgnn_updated_tail_scratch_elems(n, c, hd, no), x.device)
    check(lib().dgnn_updated_tail_bwd(n, ptr(x), _ld(x), c, ptr(W1), hd, ptr(W3), no, ptr(h), ptr(g), ptr(dW1), ptr(db1), ptr(dW3), ptr(db3), ptr(dx), ptr(dh),
                                      ptr(scratch), int(x.dtype == torch.bfloat16), GEMM_MODE, stream_ptr()), "dgnn_updated_tail_bwd")
    return dx, dW1, db1, dW3, db3


# ---- Updated variant, whole-scene inference (csrc/updated_infer.hip) -----------------------------------------------------------
def edge_chain_aggregate_supported(c_in: int, k_e: int, dtype=torch.float32) -> bool:
    """the layer shapes the one-launch form takes (dgnn_edge_chain_aggregate_supported) in the current GEMM mode"""
    return bool(lib().dgnn_edge_chain_aggregate_supported(int(c_in), int(k_e), int(dtype == torch.bfloat16), GEMM_MODE))


@on_device_of
def edge_chain_aggregate_fwd(rowptr, src, eid, n_dst, x, ea, We, be, ea_next=None, write_next=True):
    """lin_e + mean aggregate + the next layer's edge rows of one Updated conv layer in ONE launch (dgnn_edge_chain_aggregate_fwd):
    -> (a [n_dst, c_in], ea_next).  ea [E, >= k_e] in the order eid indexes (eid None: plan order); ea_next [E, >= c_in] receives relu(phi) at
    the same rows (allocated when None and write_next; left untouched when not write_next)."""
    _req(x, "x", dim=2)
    _req(ea, "ea", dim=2)
    We = _req(We, "We", dim=2).contiguous()
    be = _req(be, "be").contiguous()
    c_in, k_e = x.size(1), We.size(1)
    if We.size(0) != c_in or ea.size(1) < k_e:
        raise ValueError("lin_e weight %s does not match c_in=%d / edge rows %s" % (tuple(We.shape), c_in, tuple(ea.shape)))
    if write_next and ea_next is None:
        ea_next = torch.empty((ea.size(0), c_in), dtype=torch.float32, device=x.device)
    if ea_next is not None:
        _req(ea_next, "ea_next", dim=2)
        if ea_next.size(0) < ea.size(0) or ea_next.size(1) < c_in:
            raise ValueError("ea_next %s is smaller than [%d, %d]" % (tuple(ea_next.shape), ea.size(0), c_in))
    a = torch.empty((n_dst, c_in), dtype=torch.float32, device=x.device)
    check(lib().dgnn_edge_chain_aggregate_fwd(ptr(rowptr), ptr(src), ptr(eid), n_dst, ptr(x), _ld(x), c_in, ptr(ea), _ld(ea), k_e, ptr(We), ptr(be), ptr(a), c_in,
                                              ptr(ea_next), _ld(ea_next) if ea_next is not None else 0, int(bool(write_next)), GEMM_MODE, stream_ptr()),
          "dgnn_edge_chain_aggregate_fwd")
    return a, ea_next


@on_device_of
def updated_infer_fwd(x, edge_attr, plan_parts, layers, tail=None):
    """Every conv layer of a whole scene and the "sage+" output network in one library call (dgnn_updated_infer_fwd).  x [n, F] fp32 or bf16 rows,
    edge_attr fp32 [E, >= edge_in_0] in scene edge order, plan_parts = (rowptr, src, eid) of the scene's destination-sorted plan; `layers`: per conv
    layer a dict with edge_in, relu, We, be, Wl, bl, Wr; `tail` = (W1, b1, W3, b3) or None.
    -> (fp32 logits [n, n_out] | the last layer's rows in x's type, bit mask of the layers that ran through the one-launch form)."""
    _req(x, "x", ACT, dim=2)
    _req(edge_attr, "edge_attr", dim=2)
    dev, bf, L = x.device, x.dtype == torch.bfloat16, len(layers)
    rowptr, src, eid = plan_parts
    n, E = x.size(0), edge_attr.size(0)
    widths = [x.size(1)] + [l["Wl"].size(0) for l in layers]
    for i, l in enumerate(layers):
        if l["Wl"].size(1) != widths[i] or l["We"].size(0) != widths[i] or l["We"].size(1) != l["edge_in"]:
            raise ValueError("Updated conv %d: lin_e %s / lin_l %s do not match %d input channels, %d edge columns"
                             % (i, tuple(l["We"].shape), tuple(l["Wl"].shape), widths[i], l["edge_in"]))
    w_arr = _iarr(widths, C.c_int32)
    k_arr = _iarr([l["edge_in"] for l in layers], C.c_int32)
    r_arr = _iarr([int(bool(l["relu"])) for l in layers], C.c_int32)
    arr = lambda k: _parr([l[k] for l in layers])
    hdim = tail[0].size(0) if tail is not None else 0
    n_out = tail[2].size(0) if tail is not None else 0
    ea_cols = max(widths[:L])
    ea_buf = torch.empty((2, max(E, 1), ea_cols), dtype=x.dtype, device=dev)
    work = torch.empty(int(lib().dgnn_updated_infer_workspace_bytes(n, E, L, w_arr, k_arr, hdim, int(bf))), dtype=torch.uint8, device=dev)
    out = torch.empty((n, n_out), dtype=torch.float32, device=dev) if tail is not None else torch.empty((n, widths[-1]), dtype=x.dtype, device=dev)
    fused = C.c_int32(0)
    t = tail if tail is not None else (None,) * 4
    check(lib().dgnn_updated_infer_fwd(ptr(rowptr), ptr(src), ptr(eid), n, E, ptr(x), _ld(x), ptr(edge_attr), _ld(edge_attr), L, w_arr, k_arr,
                                       arr("We"), arr("be"), arr("Wl"), arr("bl"), arr("Wr"), r_arr, ptr(t[0]), ptr(t[1]), hdim, ptr(t[2]), ptr(t[3]), n_out,
                                       ptr(ea_buf[0]), ptr(ea_buf[1]), ptr(work), ptr(out), C.byref(fused), int(bf), GEMM_MODE, stream_ptr()),
          "dgnn_updated_infer_fwd")
    return out, int(fused.value)


# ---- edge-embedding chaining of the Updated variant (csrc/chain.hip) ---------------------------------------------------------
@on_device_of
def edge_chain_fwd(phi, e_id_cur, e_id_next, c, pos, relu):
    """-> (out [n_next, c] = relu?(zeros[E_all, C]; [e_id_cur] = phi)[e_id_next, :c], inv int32 [n_cur]); `pos`: int32 [E_all]
    table holding -1 everywhere (left that way)."""
    _req(phi, "phi", ACT, dim=2)
    _req(e_id_cur, "e_id_cur", torch.int64, 1)
    _req(e_id_next, "e_id_next", torch.int64, 1)
    _req(pos, "pos", torch.int32, 1)
    n_cur, n_next = e_id_cur.numel(), e_id_next.numel()
    if phi.size(0) != n_cur or not 0 < c <= phi.size(1):
        raise ValueError("phi %s does not match e_id_cur (%d) / c=%d" % (tuple(phi.shape), n_cur, c))
    e_id_cur, e_id_next = e_id_cur.contiguous(), e_id_next.contiguous()
    out = torch.empty((n_next, c), dtype=phi.dtype, device=phi.device)
    inv = torch.empty(max(n_cur, 1), dtype=torch.int32, device=phi.device)[:n_cur]
    check(getattr(lib(), "dgnn_edge_chain_fwd" + _sfx(phi))(ptr(phi), _ld(phi), int(c), ptr(e_id_cur), n_cur, ptr(e_id_next), n_next, pos.numel(),
                                                            ptr(pos), int(bool(relu)), ptr(out), c, ptr(inv), stream_ptr()),
          "dgnn_edge_chain_fwd", poll=True)
    return out, inv


@on_device_of
def edge_chain_bwd(g, phi, inv, c, relu):
    _req(phi, "phi", ACT, dim=2)
    _same(_req(g, "g", ACT, dim=2), phi, "g")
    dphi = torch.empty((phi.size(0), phi.size(1)), dtype=phi.dtype, device=phi.device)
    check(getattr(lib(), "dgnn_edge_chain_bwd" + _sfx(phi))(ptr(g), _ld(g), ptr(phi), _ld(phi), ptr(inv), phi.size(0), int(c), phi.size(1),
                                                            int(bool(relu)), ptr(dphi), phi.size(1), stream_ptr()), "dgnn_edge_chain_bwd")
    return dphi


# ---- volume-weighted KL cell loss (csrc/loss.hip) ------------------------------------------------------------------------------
CELL_NORMS = {None: 0, "": 0, "none": 0, "log": 1, "sqrt": 2}


@on_device_of
def kl_cell_loss_fwd(logits, gt, vol, norm: int):
    """-> (loss fp32 0-dim, sums fp64 [3] = sum cell*w, sum w, OA count)"""
    _req(logits, "logits", dim=2)
    _req(gt, "gt", dim=2)
    _req(vol, "vol", dim=1)
    n = logits.size(0)
    if logits.size(1) != 2 or gt.size(1) < 2 or gt.size(0) != n or vol.numel() != n:
        raise ValueError("kl_cell_loss: logits [n,2], gt [n,>=2], vol [n] expected, got %s %s %s" % (tuple(logits.shape), tuple(gt.shape), tuple(vol.shape)))
    out = torch.empty(4, dtype=torch.float64, device=logits.device)   # sums[3] | the fp32 loss in the first half of the 4th
    loss = out[3:].view(torch.float32)[:1].view(())
    scratch = torch.empty(int(lib().dgnn_kl_cell_loss_scratch_doubles(n)), dtype=torch.float64, device=logits.device)
    check(lib().dgnn_kl_cell_loss_fwd(ptr(logits), _ld(logits), ptr(gt), _ld(gt), ptr(vol), vol.stride(0), int(norm), n, ptr(out), ptr(loss), ptr(scratch),
                                      stream_ptr()), "dgnn_kl_cell_loss_fwd")
    return loss, out[:3]


@on_device_of
def kl_cell_loss_bwd(logits, gt, vol, norm: int, sums, grad_loss):
    dl = torch.empty((logits.size(0), 2), dtype=torch.float32, device=logits.device)
    grad_loss = grad_loss.to(torch.float32).contiguous()
    check(lib().dgnn_kl_cell_loss_bwd(ptr(logits), _ld(logits), ptr(gt), _ld(gt), ptr(vol), vol.stride(0), int(norm), logits.size(0), ptr(sums),
                                      ptr(grad_loss), ptr(dl), 2, stream_ptr()), "dgnn_kl_cell_loss_bwd")
    return dl


@on_device_of
def kl_cell_loss_step(logits, gt, vol, norm: int, running=None, grad_loss=None, backward=True):
    """kl_cell_loss_fwd + (`running` fp64 [3] += sums) + kl_cell_loss_bwd as ONE launch -> (loss, sums, dlogits | None); the same bits as the two
    calls.  None when the library declines the size (more than 65536 rows): the caller then makes the two calls."""
    _req(logits, "logits", dim=2)
    _req(gt, "gt", dim=2)
    _req(vol, "vol", dim=1)
    n = logits.size(0)
    if logits.size(1) != 2 or gt.size(1) < 2 or gt.size(0) != n or vol.numel() != n:
        raise ValueError("kl_cell_loss: logits [n,2], gt [n,>=2], vol [n] expected, got %s %s %s" % (tuple(logits.shape), tuple(gt.shape), tuple(vol.shape)))
    if running is not None and (running.dtype != torch.float64 or running.numel() < 3 or not running.is_contiguous() or running.device != logits.device):
        raise ValueError("kl_cell_loss_step: `running` must be a contiguous fp64 [3] tensor on the logits' device")
    out = torch.empty(4, dtype=torch.float64, device=logits.device)   # sums[3] | the fp32 loss in the first half of the 4th
    loss = out[3:].view(torch.float32)[:1].view(())
    dl = torch.empty((n, 2), dtype=torch.float32, device=logits.device) if backward else None
    rc = lib().dgnn_kl_cell_loss_step(ptr(logits), _ld(logits), ptr(gt), _ld(gt), ptr(vol), vol.stride(0), int(norm), n, ptr(grad_loss), ptr(out), ptr(loss),
                                      ptr(running), ptr(dl), 2, stream_ptr())
    if rc == DGNN_E_UNSUPPORTED:
        return None
    check(rc, "dgnn_kl_cell_loss_step")
    return loss, out[:3], dl


# ---- edge total-variation regulariser (csrc/edge_tv.hip) -------------------------------------------------------------------------
def _edge_tv_args(logits, edge_index, what):
    """-> (src pointer, dst pointer, element stride, idx64, E) of a PyG-style [2, E] int32 / int64 edge_index as it lies in memory (a column slice of
    a larger one and the transposed view of an [E, 2] array included); nothing is converted or copied"""
    _req(logits, "logits", dim=2)
    if logits.size(1) != 2 or logits.size(0) == 0:
        raise ValueError("%s: logits [n, 2] with n >= 1 expected, got %s" % (what, tuple(logits.shape)))
    if not isinstance(edge_index, torch.Tensor):
        raise TypeError("edge_index must be a tensor")
    if edge_index.device != logits.device:
        raise DgnnError("edge_index is on %s, the logits on %s" % (edge_index.device, logits.device))
    if edge_index.dtype not in (torch.int32, torch.int64):
        raise TypeError("edge_index must be int32 or int64, got %s" % edge_index.dtype)
    if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.size(1) < 1:
        raise ValueError("%s: edge_index [2, E] with E >= 1 expected, got %s" % (what, tuple(edge_index.shape)))
    es = edge_index.stride(1) if edge_index.size(1) > 1 else 1
    if es < 1 or edge_index.stride(0) < 0:
        raise ValueError("edge_index must have positive strides (stride %s)" % (edge_index.stride(),))
    p0 = edge_index.data_ptr()
    return C.c_void_p(p0), C.c_void_p(p0 + edge_index.stride(0) * edge_index.element_size()), es, int(edge_index.dtype == torch.int64), edge_index.size(1)


def _edge_tv_out(device, total):
    """sums fp64 [2] | reg (| total) fp32 in the third double of one allocation"""
    out = torch.empty(3, dtype=torch.float64, device=device)
    f = out[2:].view(torch.float32)
    return out[:2], f[0], (f[1] if total else None)


def _edge_tv_scratch(device):
    return torch.empty(int(lib().dgnn_edge_tv_scratch_doubles()), dtype=torch.float64, device=device)


@on_device_of
def edge_tv_fwd(logits, edge_index, weight: float, need_grad=True, max_blocks=None):
    """-> (reg fp32 0-dim = weight * sum_e |p(src_e) - p(dst_e)| / E, sums fp64 [2] = (weight * sum tv, E), net int32 [n] | None) with
    p = softmax(logits)[:, 0]; `net` (need_grad) holds the signed edge counts edge_tv_bwd turns into the gradient.  Indices are < n by contract.
    max_blocks: a cap on the edge pass's workgroups (None: the library's)."""
    src, dst, es, idx64, E = _edge_tv_args(logits, edge_index, "edge_tv_fwd")
    n = logits.size(0)
    sums, reg, _ = _edge_tv_out(logits.device, False)
    net = torch.empty(n, dtype=torch.int32, device=logits.device) if need_grad else None
    check(lib().dgnn_edge_tv_fwd(ptr(logits), _ld(logits), n, src, dst, es, idx64, E, float(weight), ptr(net), ptr(sums), ptr(reg), ptr(_edge_tv_scratch(logits.device)),
                                 int(max_blocks or 0), stream_ptr()), "dgnn_edge_tv_fwd", poll=True)
    return reg, sums, net


@on_device_of
def edge_tv_bwd(logits, net, weight: float, E: int, grad_loss=None, out=None):
    """dlogits [n, 2] of edge_tv_fwd's `reg` (times the 0-dim `grad_loss`, None = 1) from its `net`; `out`: fp32 [n, 2] rows the gradient is ADDED to"""
    _req(logits, "logits", dim=2)
    n = logits.size(0)
    if logits.size(1) != 2 or net.dtype != torch.int32 or net.numel() < n or not net.is_contiguous() or net.device != logits.device or E < 1:
        raise ValueError("edge_tv_bwd: logits [n, 2], net int32 [n] of edge_tv_fwd and its E expected")
    if out is not None and (_req(out, "out", dim=2).shape != logits.shape):
        raise ValueError("edge_tv_bwd: `out` must have the logits' shape")
    if grad_loss is not None:
        grad_loss = grad_loss.to(torch.float32).contiguous()
    dl = out if out is not None else torch.empty((n, 2), dtype=torch.float32, device=logits.device)
    check(lib().dgnn_edge_tv_bwd(ptr(logits), _ld(logits), n, ptr(net), float(weight), int(E), ptr(grad_loss), ptr(dl), _ld(dl), int(out is not None), stream_ptr()),
          "dgnn_edge_tv_bwd")
    return dl


_tv_net = {}      # (device, stream) -> zeroed int32 table of edge_tv_step (the finish pass hands it back zeroed: no memset launch per step)


@on_device_of
def edge_tv_step(logits, edge_index, weight: float, grad_loss=None, add_loss=None, running=None, dlogits=None, max_blocks=None):
    """edge_tv_fwd + edge_tv_bwd as TWO launches -> (reg, sums, dlogits, total): the same bits as the two calls.  `dlogits`: fp32 [n, 2] rows the
    gradient is ADDED to (the KL loss's; None: a fresh tensor is written); `add_loss`: fp32 0-dim, total = add_loss + reg comes back (else None);
    `running`: fp64 [2] accumulator, += sums in the same launch.  The signed-count table is kept per device AND stream between calls: calls on one
    stream are ordered, calls on different streams use different tables."""
    src, dst, es, idx64, E = _edge_tv_args(logits, edge_index, "edge_tv_step")
    n, dev = logits.size(0), logits.device
    if dlogits is not None and _req(dlogits, "dlogits", dim=2).shape != logits.shape:
        raise ValueError("edge_tv_step: `dlogits` must have the logits' shape")
    if running is not None and (running.dtype != torch.float64 or running.numel() < 2 or not running.is_contiguous() or running.device != dev):
        raise ValueError("edge_tv_step: `running` must be a contiguous fp64 [2] tensor on the logits' device")
    if add_loss is not None and (add_loss.dtype != torch.float32 or add_loss.numel() != 1 or add_loss.device != dev):
        raise ValueError("edge_tv_step: `add_loss` must be one fp32 value on the logits' device")
    if grad_loss is not None:
        grad_loss = grad_loss.to(torch.float32).contiguous()
    stream = stream_ptr()
    key = (dev, stream.value)
    net = _tv_net.get(key)
    if net is None or net.numel() < n:
        net = _tv_net[key] = torch.zeros(max(1 << 16, 1 << (n - 1).bit_length()), dtype=torch.int32, device=dev)
    sums, reg, total = _edge_tv_out(dev, add_loss is not None)
    dl = dlogits if dlogits is not None else torch.empty((n, 2), dtype=torch.float32, device=dev)
    try:
        check(lib().dgnn_edge_tv_step(ptr(logits), _ld(logits), n, src, dst, es, idx64, E, float(weight), ptr(grad_loss), ptr(net), 1, ptr(sums), ptr(reg), ptr(add_loss),
                                      ptr(total), ptr(running), ptr(dl), _ld(dl), int(dlogits is not None), ptr(_edge_tv_scratch(dev)), int(max_blocks or 0),
                                      stream), "dgnn_edge_tv_step", poll=True)
    except Exception:
        _tv_net.pop(key, None)      # (a failed call may leave counts behind: the next one starts from a fresh zeroed table)
        raise
    return reg, sums, dl, total


# ---- Updated variant: one conv layer per call each way (csrc/train.hip) --------------------------------------------------------
@on_device_of
def sage_updated_train_fwd(plan_parts, n_dst, x, ea, We, be, Wl, bl, Wr, relu):
    """-> (y [n_dst,c_out], phi [E,c_in], a [n_dst,c_in]) in the storage type of x (fp32 or bf16)"""
    _req(x, "x", ACT, dim=2)
    _same(_req(ea, "edge_attr", ACT, dim=2), x, "edge_attr")
    rowptr, src, eid = plan_parts
    c_in, c_out, k_e, E = x.size(1), Wl.size(0), We.size(1), ea.size(0)
    if We.size(0) != c_in or ea.size(1) != k_e or Wl.size(1) != c_in:
        raise ValueError("Updated conv: lin_e %s / lin_l %s do not match x %s, edge_attr %s" % (tuple(We.shape), tuple(Wl.shape), tuple(x.shape), tuple(ea.shape)))
    phi = torch.empty((E, c_in), dtype=x.dtype, device=x.device)
    a = torch.empty((n_dst, c_in), dtype=x.dtype, device=x.device)
    y = torch.empty((n_dst, c_out), dtype=x.dtype, device=x.device)
    check(lib().dgnn_sage_updated_train_fwd(ptr(rowptr), ptr(src), ptr(eid), n_dst, ptr(x), _ld(x), c_in, ptr(ea), _ld(ea), k_e, E, ptr(We), ptr(be), ptr(Wl),
                                            ptr(bl), ptr(Wr), c_out, int(bool(relu)), ptr(phi), ptr(a), ptr(y), int(x.dtype == torch.bfloat16), GEMM_MODE,
                                            stream_ptr()), "dgnn_sage_updated_train_fwd")
    return y, phi, a


@on_device_of
def sage_updated_train_bwd(t_parts, rowptr_dst, n_src, n_dst, x, ea, We, Wl, Wr, has_bias, relu, phi, a, y, dy, dphi_ext, need_dx, need_dea):
    """-> (dx | None, d_ea | None, dWe, dbe, dWl, dbl | None, dWr | None); parameter gradients are views of one fp32 buffer"""
    c_in, c_out, k_e, E = x.size(1), Wl.size(0), We.size(1), ea.size(0)
    dev, dt = x.device, x.dtype
    _, _, ((dWe, dbe, dWl, dbl, dWr),) = _grad_buffer([[(c_in, k_e), (c_in,), (c_out, c_in), (c_out,) if has_bias else None,
                                                         (c_out, c_in) if Wr is not None else None]], dev)
    dx = torch.empty((n_src, c_in), dtype=dt, device=dev) if need_dx else None
    d_ea = torch.empty((E, k_e), dtype=dt, device=dev) if need_dea else None
    dz = torch.empty((n_dst, c_out), dtype=dt, device=dev) if relu else None
    da = torch.empty((n_dst, 2 * c_in), dtype=dt, device=dev)     # [da | dz . Wr] of the merged input-gradient GEMM
    dphi = torch.empty((max(E, 1), c_in), dtype=dt, device=dev)
    scratch = _f32(lib().dgnn_sage_updated_train_scratch_elems(n_dst, E, c_in, c_out, k_e), dev)
    t_rowptr, t_dst, t_eid = t_parts
    check(lib().dgnn_sage_updated_train_bwd(ptr(t_rowptr), ptr(t_dst), ptr(t_eid), ptr(rowptr_dst), n_src, n_dst, E, ptr(x), _ld(x), c_in, ptr(ea), _ld(ea), k_e,
                                            ptr(We), ptr(Wl), ptr(Wr), c_out, int(bool(relu)), ptr(phi), ptr(a), ptr(y), ptr(dy), ptr(dphi_ext), ptr(dx), ptr(d_ea),
                                            ptr(dWe), ptr(dbe), ptr(dWl), ptr(dbl), ptr(dWr), ptr(dz), ptr(da), ptr(dphi), ptr(scratch),
                                            int(dt == torch.bfloat16), GEMM_MODE, stream_ptr()), "dgnn_sage_updated_train_bwd")
    return (dx, d_ea, dWe, dbe, dWl, dbl, dWr)


# ---- Static model in training mode, all layers per call (csrc/train.hip) -------------------------------------------------------
def _parr(vals):
    return (C.c_void_p * len(vals))(*[(v.data_ptr() if isinstance(v, torch.Tensor) else v) for v in vals])


def _iarr(vals, ty):
    return (ty * len(vals))(*vals)


_PARAM_ARRAYS = {}      # pointer tables of a model's parameters and BatchNorm buffers, rebuilt only when one of the pointers has moved


def _param_arrays(layers):
    """ctypes tables (one entry per layer) of everything in `layers` that belongs to the MODEL, not to the batch: built once and reused while
    the tensors keep their addresses (40 data_ptr() reads a step instead of a dozen table constructions)."""
    names = ("We", "be", "Wj", "bj", "Wi", "gamma", "beta")
    key = tuple((l[k].data_ptr() if l[k] is not None else 0) for l in layers for k in names) + tuple(
        ((bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr() if bn.track_running_stats else 0, bn.momentum, bn.eps)
         if bn is not None else None) for bn in (l["bn"] for l in layers))
    hit = _PARAM_ARRAYS.get(len(layers))
    if hit is not None and hit[0] == key:
        return hit[1]
    t = {k: _parr([l[k] for l in layers]) for k in names}
    bns = [l["bn"] for l in layers]
    t["rm"] = _parr([(bn.running_mean if bn is not None else None) for bn in bns])
    t["rv"] = _parr([(bn.running_var if bn is not None else None) for bn in bns])
    t["nbt"] = _parr([(bn.num_batches_tracked if bn is not None and bn.track_running_stats else None) for bn in bns])
    t["momentum"] = _iarr([(bn.momentum if bn is not None else 0.0) for bn in bns], C.c_float)
    t["eps"] = _iarr([(bn.eps if bn is not None else 0.0) for bn in bns], C.c_float)
    _PARAM_ARRAYS[len(layers)] = (key, t)
    return t


@on_device_of
def static_train_fwd(x0, layers):
    """`layers`: list of dicts (one per conv layer, then optionally the decoder's Linear + BN block with plan None) with keys
    plan_parts (rowptr, src, eid) | None, n_dst, edge_attr | None, We, be, Wj, bj, Wi, gamma, beta, bn.
    -> (y_last, buf, meta): one fp32 buffer holding every layer's a / z / y / stats, `meta` the element offsets."""
    _req(x0, "x", dim=2)
    dev, L = x0.device, len(layers)
    widths = [x0.size(1)] + [l["Wj"].size(0) for l in layers]
    meta, off = [], 0
    for i, l in enumerate(layers):
        n, ci, co = l["n_dst"], widths[i], widths[i + 1]
        if l["Wj"].size(1) != ci:
            raise ValueError("layer %d: lin_j %s does not take %d channels" % (i, tuple(l["Wj"].shape), ci))
        m = dict(a=off if l["plan_parts"] is not None else None)
        off += n * ci if l["plan_parts"] is not None else 0
        if l["bn"] is None:      # a plain Linear (the decoder's output layer): y only
            m["z"] = m["stats"] = None
            m["y"], off = off, off + n * co
        else:
            m["z"], off = off, off + n * co
            m["y"], off = off, off + n * co
            m["stats"], off = off, off + 4 * co
        meta.append(m)
    buf = _f32_work(off, dev)
    base = buf.data_ptr()
    at = lambda o: None if o is None else base + 4 * o
    scratch = _f32_work(max(lib().dgnn_colstats_scratch_elems(l["n_dst"], widths[i + 1]) for i, l in enumerate(layers)) + 2, dev)
    pp = lambda k: _parr([(l["plan_parts"][k] if l["plan_parts"] is not None else None) for l in layers])
    key = lambda k: _parr([l[k] for l in layers])
    f_e = max([l["We"].size(1) for l in layers if l["We"] is not None] or [0])
    pa = _param_arrays(layers)
    check(lib().dgnn_static_train_fwd(
        L, pp(0), pp(1), pp(2), _iarr([l["n_dst"] for l in layers], C.c_int64), ptr(x0), _ld(x0), _iarr(widths, C.c_int32),
        key("edge_attr"), _iarr([(_ld(l["edge_attr"]) if l["edge_attr"] is not None else 0) for l in layers], C.c_int64), f_e,
        pa["We"], pa["be"], pa["Wj"], pa["bj"], pa["Wi"], pa["gamma"], pa["beta"], pa["rm"], pa["rv"], pa["nbt"], pa["momentum"], pa["eps"],
        _parr([at(m["a"]) for m in meta]), _parr([at(m["z"]) for m in meta]), _parr([at(m["stats"]) for m in meta]), _parr([at(m["y"]) for m in meta]),
        ptr(scratch), GEMM_MODE, stream_ptr()), "dgnn_static_train_fwd")
    _written_behind_torch(*[t for l in layers if l["bn"] is not None
                            for t in (l["bn"].running_mean, l["bn"].running_var, l["bn"].num_batches_tracked if l["bn"].track_running_stats else None)])
    n, co = layers[-1]["n_dst"], widths[-1]
    return torch.as_strided(buf, (n, co), (co, 1), meta[-1]["y"]), buf, (meta, widths, pa)


@on_device_of
def static_train_bwd(x0, layers, buf, meta_widths, dy, keep=None):
    """-> per-layer parameter gradients [(dWe, dbe, dWj, dbj, dWi, dgamma, dbeta), ...] (views of one buffer; None where the layer has
    no such parameter).  `keep`: a dict owned by the caller (the model) -- the gradient buffer and its views are then made ONCE and every step writes
    into the same tensors (round 6: one allocation and 34 view ops a step less; what the optimizer reads through p.grad stays at one address)."""
    meta, widths, pa = meta_widths
    dev, L = x0.device, len(layers)
    base = buf.data_ptr()
    at = lambda o: None if o is None else base + 4 * o
    kept = keep.get("static_bwd") if keep is not None else None
    sig = (dev, tuple(widths), tuple((l["We"].size(1) if l["We"] is not None else 0, l["bj"] is not None, l["Wi"] is not None, l["bn"] is not None) for l in layers))
    if kept is not None and kept[0] == sig:
        _, goffs, flat, grads = kept
    else:
        rows = []
        for i, l in enumerate(layers):
            ci, co = widths[i], widths[i + 1]
            fe = l["We"].size(1) if l["We"] is not None else 0
            bn = (co,) if l["bn"] is not None else None
            rows.append([(ci, fe), (ci,) if fe else None, (co, ci), (co,) if l["bj"] is not None else None, (co, ci) if l["Wi"] is not None else None, bn, bn])
        flat, goffs, grads = _grad_buffer(rows, dev)
        if keep is not None:
            keep["static_bwd"] = (sig, goffs, flat, grads)
    gbase = flat.data_ptr()
    gat = lambda o: None if o is None else gbase + 4 * o
    n_src = [(l["n_src"] if l["plan_parts"] is not None else l["n_dst"]) for l in layers]
    dxn = max([n_src[i] * widths[i] for i in range(1, L)] or [1])
    dxn = (dxn + (1 << 20) - 1) >> 20 << 20
    dxb = torch.empty((2, dxn), dtype=torch.float32, device=dev)
    f_e = max([l["We"].size(1) for l in layers if l["We"] is not None] or [0])
    scratch = _f32_work(lib().dgnn_static_train_scratch_elems(L, _iarr(n_src, C.c_int64), _iarr([l["n_dst"] for l in layers], C.c_int64),
                                                              _iarr(widths, C.c_int32), f_e), dev)
    tp = lambda k: _parr([(l["t_parts"][k] if l["plan_parts"] is not None else None) for l in layers])
    key = lambda k: _parr([l[k] for l in layers])
    col = lambda j: _parr([gat(r[j]) for r in goffs])
    check(lib().dgnn_static_train_bwd(
        L, tp(0), tp(1), tp(2), _parr([(l["plan_parts"][0] if l["plan_parts"] is not None else None) for l in layers]), _iarr(n_src, C.c_int64),
        _iarr([l["n_dst"] for l in layers], C.c_int64), ptr(x0), _ld(x0), _iarr(widths, C.c_int32), key("edge_attr"),
        _iarr([(_ld(l["edge_attr"]) if l["edge_attr"] is not None else 0) for l in layers], C.c_int64), f_e, pa["We"], pa["be"], pa["Wj"], pa["Wi"],
        pa["gamma"], _parr([at(m["stats"]) for m in meta]), pa["eps"], _parr([at(m["a"]) for m in meta]),
        _parr([at(m["z"]) for m in meta]), _parr([at(m["y"]) for m in meta]), ptr(dy), col(0), col(1), col(2), col(3), col(4), col(5), col(6),
        _parr([dxb[0], dxb[1]]), ptr(scratch), GEMM_MODE, stream_ptr()), "dgnn_static_train_bwd")
    return grads


# ---- graph cut (reference processing/generate_mesh.py:15-58) ----------------------------------------------------------------------
def potts_weight(binary_weight) -> int:
    """The Potts weight as the reference's `np.ones(n, int64) * binary_weight` reaches gco's integer costs (truncation); ValueError when
    it is negative (not a cut problem) or does not fit int32."""
    import numpy as np

    bw = float(binary_weight)
    if not np.isfinite(bw) or bw < 0:
        raise ValueError("graph cut: binary_weight %r must be finite and >= 0" % (binary_weight,))
    w = int(np.trunc(bw))
    if w > 0x7FFFFFFF:
        raise ValueError("graph cut: binary_weight %r does not fit int32" % (binary_weight,))
    return w


def _cut_arrays(logits, edges):
    """the inputs of a graph cut on their device, then n, F and its output arrays: labels [n], (energy, flow) int64, (steps, relabels) int32"""
    dev = logits.device if isinstance(logits, torch.Tensor) and logits.is_cuda else torch.device("cuda", torch.cuda.current_device())
    logits = torch.as_tensor(logits).to(dev, torch.float32)
    edges = torch.as_tensor(edges).to(dev, torch.int32).contiguous()
    if logits.dim() != 2 or logits.size(1) != 2:
        raise ValueError("logits must be [n, 2], got %s" % (tuple(logits.shape),))
    if edges.numel() == 0:
        edges = edges.reshape(0, 2)
    if edges.dim() != 2 or edges.size(1) != 2:
        raise ValueError("edges must be [F, 2], got %s" % (tuple(edges.shape),))
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    n = logits.size(0)
    return (dev, logits, edges, n, edges.size(0), _empty(dev, torch.int32, n), torch.zeros(2, dtype=torch.int64, device=dev),
            torch.zeros(2, dtype=torch.int32, device=dev))


def _cut_result(labels, out64, stats, return_stats):
    energy, flow = (int(v) for v in out64.cpu())
    return (labels, energy, flow, _stats_dict(("steps", "relabels"), stats)) if return_stats else (labels, energy, flow)


@on_device_of
def binary_graph_cut(logits, edges, unary_weight, binary_weight, return_stats=False):
    """Exact minimum of the reference's two-label graph-cut energy (dgnn_graph_cut_binary):
    D_i(0) = round(logits[i,1] * uw), D_i(1) = round(logits[i,0] * uw) in fp32, Potts weight `binary_weight` per row of `edges`.
    logits fp32 [n, 2], edges int [F, 2] (tensors or arrays; CPU inputs are moved to the GPU).
    -> (labels int32 [n] on the GPU: 0 inside / 1 outside, the minimiser with the fewest outside cells; energy int; max-flow value int)
    (+ {"steps", "relabels"} with return_stats).  Raises ValueError for a negative weight, DgnnError for an edge id outside [0, n),
    non-finite logits, |cost| >= 2^30 or capacities that overflow int32."""

    w = potts_weight(binary_weight)
    dev, logits, edges, n, f, labels, out64, stats = _cut_arrays(logits, edges)
    scratch = _scratch(dev, lib().dgnn_graph_cut_scratch_bytes(n, f))
    check(lib().dgnn_graph_cut_binary(ptr(logits), max(_ld(logits), 2) if n else 2, n, ptr(edges), f, float(unary_weight), w, ptr(labels),
                                      ptr(out64), C.c_void_p(out64.data_ptr() + 8), ptr(stats), ptr(scratch), stream_ptr()), "dgnn_graph_cut_binary")
    return _cut_result(labels, out64, stats, return_stats)


@on_device_of
def weighted_graph_cut(logits, edges, unary_weight, row_weights, return_stats=False):
    """`binary_graph_cut` with one integer capacity per row of `edges` (dgnn_graph_cut_weighted): the exact minimum of
    sum_i D_i(l_i) + sum_r row_weights[r] [l_i != l_j].  row_weights int [F], each >= 0 (e.g. from facet_cut_terms, compacted to the
    finite-finite rows); a row of weight 0 carries nothing, duplicate rows add up, self-loops never count.  Returns what
    binary_graph_cut returns; with every weight equal to w, exactly what binary_graph_cut(..., w) returns (steps and relabels too).
    Raises ValueError for a wrong length or shape, DgnnError for a negative weight, capacities that overflow int32 and what
    binary_graph_cut raises."""
    dev, logits, edges, n, f, labels, out64, stats = _cut_arrays(logits, edges)
    rw = torch.as_tensor(row_weights)
    if rw.is_floating_point() or rw.dtype == torch.bool:
        raise ValueError("row_weights must be integers, got %s" % (rw.dtype,))
    if rw.dim() != 1 or rw.numel() != edges.size(0):
        raise ValueError("row_weights must be [%d] (one per row of edges), got %s" % (edges.size(0), tuple(rw.shape)))
    if rw.dtype == torch.int64 and rw.numel() and (int(rw.max()) > 0x7FFFFFFF or int(rw.min()) < -0x80000000):   # narrower types fit
        raise ValueError("row_weights do not fit int32")
    rw = rw.to(dev, torch.int32).contiguous()
    scratch = _scratch(dev, lib().dgnn_graph_cut_weighted_scratch_bytes(n, f))
    check(lib().dgnn_graph_cut_weighted(ptr(logits), max(_ld(logits), 2) if n else 2, n, ptr(edges), f, float(unary_weight), ptr(rw), ptr(labels),
                                        ptr(out64), C.c_void_p(out64.data_ptr() + 8), ptr(stats), ptr(scratch), stream_ptr()),
          "dgnn_graph_cut_weighted")
    return _cut_result(labels, out64, stats, return_stats)


CUT_TERM_KINDS = {"area": 1, "beta": 2}


@on_device_of
def facet_cut_terms(vertices, tetrahedra, facets, nfacets, kind, binary_weight, return_q=False):
    """Integer graph-cut capacities of the facets of `<scene>_3dt.npz` from their geometry (dgnn_facet_cut_terms):
    kind "area": q_f = A_f / mean(A); kind "beta": q_f = 1 - min(cos phi, cos psi) of the two cells' circumspheres (Labatut et al. 2009);
    w_f = rint(binary_weight * q_f).  Only facets between two finite cells (both nfacets entries >= 0) are weighted; the others get 0.
    vertices fp64 [V, 3], tetrahedra int [N, 4], facets int [F, 3], nfacets int [F, 2].
    -> (w int32 [F] on the GPU, stats {"rows", "neutral_sides", "zero_weights", "max_weight"}), with return_q (w, q fp64 [F], stats).
    ValueError for an unknown kind or a binary_weight that is negative or not finite; DgnnError for malformed input, a mean area of 0
    and weights that reach 2^30."""
    import numpy as np

    if kind not in CUT_TERM_KINDS:
        raise ValueError("facet_cut_terms: kind %r (expected \"area\" or \"beta\")" % (kind,))
    bw = float(binary_weight)
    if not np.isfinite(bw) or bw < 0:
        raise ValueError("facet_cut_terms: binary_weight %r must be finite and >= 0" % (binary_weight,))
    dev = _dev_of(vertices, tetrahedra, facets, nfacets)
    v, tets, fac, nfac = _scene(dev, vertices, tetrahedra, facets, nfacets)
    f = fac.size(0)
    w = _empty(dev, torch.int32, f)
    q = _empty(dev, torch.float64, f) if return_q else None
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    scratch = _scratch(dev, lib().dgnn_facet_cut_terms_scratch_bytes(f))
    check(lib().dgnn_facet_cut_terms(ptr(v), v.size(0), ptr(tets), tets.size(0), ptr(fac), ptr(nfac), f, CUT_TERM_KINDS[kind], bw, ptr(q), ptr(w),
                                     ptr(stats), ptr(scratch), stream_ptr()), "dgnn_facet_cut_terms")
    sd = _stats_dict(("rows", "neutral_sides", "zero_weights", "max_weight"), stats)
    return (w, q, sd) if return_q else (w, sd)


# ---- mesh metrics (reference processing/generate_mesh.py:126-163, processing/evaluate_mesh.py) ----------------------------------
def _dev_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _on(x, dev, dtype, cols=None):
    t = torch.as_tensor(x).to(dev, dtype).contiguous()
    if cols is not None:
        if t.numel() == 0:
            t = t.reshape(0, cols)
        if t.dim() != 2 or t.size(1) != cols:
            raise ValueError("expected [n, %d], got %s" % (cols, tuple(t.shape)))
    return t


def _empty(dev, dtype, *shape):
    n = 1
    for s in shape:
        n *= s
    return torch.empty(max(n, 1), dtype=dtype, device=dev)[:n].view(*shape)


def _zeros(dev, dtype, n):
    """n zeros in a storage of at least one element (its pointer is never null)"""
    return torch.zeros(max(n, 1), dtype=dtype, device=dev)[:n]


def _scratch(dev, nbytes, overflow=None, or_one=False):
    """`nbytes` of workspace.  overflow: the DgnnError for a size <= 0 (beyond the int32 indexing); or_one: a byte at least: the call refuses"""
    nbytes = int(nbytes)
    if overflow is not None and nbytes <= 0:
        raise DgnnError(overflow)
    return torch.empty(max(nbytes, 1) if or_one else nbytes, dtype=torch.uint8, device=dev)


def _stats_dict(keys, stats):
    """keys -> int, from a stats tensor or a ctypes array"""
    return dict(zip(keys, (int(x) for x in (stats.cpu() if isinstance(stats, torch.Tensor) else stats))))


def _scene(dev, vertices, tetrahedra, facets, nfacets):
    """the arrays of a `<scene>_3dt.npz` on `dev`: vertices fp64 [V, 3] (None when not given), tetrahedra [T, 4], facets [F, 3], nfacets [F, 2] int32"""
    v = None if vertices is None else _on(vertices, dev, torch.float64, 3)
    tets = _on(tetrahedra, dev, torch.int32, 4)
    fac = _on(facets, dev, torch.int32, 3)
    nfac = _on(nfacets, dev, torch.int32, 2)
    if fac.size(0) != nfac.size(0):
        raise ValueError("%d facets but %d nfacets rows" % (fac.size(0), nfac.size(0)))
    return v, tets, fac, nfac


def _ray_inputs(vertices, tetrahedra, ray_vertex, sensors, incidence):
    """what the two ray operations take, on its device; (rowptr, entries) is the pair of vertex_incidence, built here when `incidence` is None"""
    dev = _dev_of(ray_vertex, sensors, vertices, tetrahedra)
    v = _on(vertices, dev, torch.float64, 3)
    tets = _on(tetrahedra, dev, torch.int32, 4)
    rv = _on(ray_vertex, dev, torch.int32).reshape(-1)
    s = _on(sensors, dev, torch.float64, 3)
    if s.size(0) != rv.numel():
        raise ValueError("%d sensor positions for %d rays" % (s.size(0), rv.numel()))
    t, nv = tets.size(0), v.size(0)
    rowptr, entries = vertex_incidence(tets, nv) if incidence is None else (_on(incidence[0], dev, torch.int32), _on(incidence[1], dev, torch.int32))
    if rowptr.numel() != nv + 1 or entries.numel() != 4 * t:
        raise ValueError("incidence of %d vertices and %d corners for %d vertices and %d tets" % (rowptr.numel() - 1, entries.numel(), nv, t))
    return dev, v, tets, rv, s, rowptr, entries


def _side_columns(out, name, count, stat, stat_names=("",)):
    """out["<side>_<name>_count"] = count[side] and out["<side>_<name>_<stat name>{min,max,sum}"] = stat[side, 3 i + j] for the i-th stat name"""
    for i, side in enumerate(RAY_SIDES):
        out["%s_%s_count" % (side, name)] = count[i]
        for a, prefix in enumerate(stat_names):
            for j, fold in enumerate(("min", "max", "sum")):
                out["%s_%s_%s%s" % (side, name, prefix, fold)] = stat[i, 3 * a + j]


@on_device_of
def locate_points(vertices, tetrahedra, facets, nfacets, points, return_steps=False):
    """The finite cell of `<scene>_3dt.npz` that contains each point (dgnn_locate_points): vertices fp64 [V, 3], tetrahedra int [N, 4],
    facets int [F, 3], nfacets int [F, 2] (-1 = infinite cell), points [P, 3] (cast to fp32).  -> int32 [P] on the GPU, -1 = outside the
    convex hull (+ the longest walk with return_steps).  Points on a shared face / vertex get the first cell of the walk that has them on
    its boundary (include/dgnn_hip.h).  DgnnError for malformed input or a walk that hits the step cap."""
    dev = _dev_of(points, vertices)
    v, tets, fac, nfac = _scene(dev, vertices, tetrahedra, facets, nfacets)
    pts = _on(points, dev, torch.float32, 3)
    n_p, n_c = pts.size(0), tets.size(0)
    cells = _empty(dev, torch.int32, n_p)
    steps = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = _scratch(dev, lib().dgnn_locate_scratch_bytes(n_c))
    check(lib().dgnn_locate_points(ptr(v), v.size(0), ptr(tets), n_c, ptr(fac), ptr(nfac), fac.size(0), ptr(pts), n_p, ptr(cells), ptr(steps),
                                   ptr(scratch), stream_ptr()), "dgnn_locate_points")
    return (cells, int(steps.item())) if return_steps else cells


@on_device_of
def iou_counts(cells, labels, occ_gt):
    """(occupancy int32 [P] on the GPU: 1 = inside = cells[i] >= 0 with labels[cells[i]] == 0; |A n B|; |A u B|) against the ground-truth
    occupancies occ_gt [P] (non-zero = inside) (dgnn_mesh_iou_counts)."""
    dev = _dev_of(cells, labels)
    cells = _on(cells, dev, torch.int32)
    labels = _on(labels, dev, torch.int32)
    occ = _on(occ_gt, dev, torch.bool).view(torch.uint8)
    if occ.numel() != cells.numel():
        raise ValueError("%d occupancies for %d points" % (occ.numel(), cells.numel()))
    n = cells.numel()
    out = _empty(dev, torch.int32, n)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    scratch = _scratch(dev, 256)
    check(lib().dgnn_mesh_iou_counts(ptr(cells), n, ptr(labels), labels.numel(), ptr(occ), ptr(out), ptr(counts), ptr(scratch), stream_ptr()),
          "dgnn_mesh_iou_counts")
    inter, union = (int(c) for c in counts.cpu())
    return out, inter, union


def mesh_iou(vertices, tetrahedra, facets, nfacets, labels, points, occ_gt):
    """IoU of the reconstructed surface (the facets between inside (label 0) and outside cells, the infinite cell outside) with the
    ground-truth occupancies, as compute_iou computes it: float32(|A n B|) / float32(|A u B|) (nan for an empty union).  Runs on the
    device of the first GPU tensor among labels, points, vertices.
    -> (iou float, occupancy int32 [P] on the GPU, |A n B|, |A u B|)."""
    import numpy as np

    dev = _dev_of(labels, points, vertices)          # the work goes where the labels are (not the thread's current device)
    cells = locate_points(vertices, tetrahedra, facets, nfacets, torch.as_tensor(points).to(dev))
    occ, inter, union = iou_counts(cells, labels, occ_gt)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = float(np.float32(inter) / np.float32(union))
    return iou, occ, inter, union


@on_device_of
def sample_interface(vertices, facets, face_ids, n_samples, seed=0, return_cum=False):
    """n_samples fp32 points [n, 3] on the GPU drawn on the faces facets[face_ids] by area (dgnn_sample_faces; the hash and the barycentric
    map are in include/dgnn_hip.h) and the position in face_ids of each sample's face (int32).  face_ids None = every facet.  With
    return_cum also the fp64 cumulative areas.  DgnnError when samples are asked of faces with no area."""
    dev = _dev_of(face_ids, vertices)
    v = _on(vertices, dev, torch.float64, 3)
    fac = _on(facets, dev, torch.int32, 3)
    ids = None if face_ids is None else _on(face_ids, dev, torch.int32).reshape(-1)
    nfc = fac.size(0) if ids is None else ids.numel()
    n = int(n_samples)
    pts = _empty(dev, torch.float32, n, 3)
    face = _empty(dev, torch.int32, n)
    cum = _empty(dev, torch.float64, nfc)
    scratch = _scratch(dev, lib().dgnn_sample_faces_scratch_bytes(nfc))
    check(lib().dgnn_sample_faces(ptr(v), v.size(0), ptr(fac), fac.size(0), ptr(ids), nfc, n, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(pts), ptr(face),
                                  ptr(cum) if nfc else None, ptr(scratch), stream_ptr()), "dgnn_sample_faces")
    return (pts, face, cum) if return_cum else (pts, face)


@on_device_of
def nearest_neighbor(ref, query):
    """Exact nearest neighbour of every query point among `ref` (both cast to fp32 [n, 3]; dgnn_nearest_neighbor): (dist fp32 [Q], index
    int32 [Q], sum of dist in fp64 in a fixed order) -- d2 = (dx*dx + dy*dy) + dz*dz in fp32, ties to the smaller index, dist = sqrtf(d2)."""
    dev = _dev_of(query, ref)
    r = _on(ref, dev, torch.float32, 3)
    q = _on(query, dev, torch.float32, 3)
    nr, nq = r.size(0), q.size(0)
    if nr == 0:
        raise ValueError("nearest_neighbor: the reference set is empty")
    dist = _empty(dev, torch.float32, nq)
    idx = _empty(dev, torch.int32, nq)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    scratch = _scratch(dev, lib().dgnn_nearest_scratch_bytes(nr, nq))
    check(lib().dgnn_nearest_neighbor(ptr(r), nr, ptr(q), nq, ptr(dist), ptr(idx), ptr(total), ptr(scratch), stream_ptr()), "dgnn_nearest_neighbor")
    return dist, idx, float(total.item())


def chamfer_distance(gt_points, recon_points):
    """compute_chamfer (processing/evaluate_mesh.py): (mean NN distance gt -> recon + mean NN distance recon -> gt) / 2, each mean an fp64
    sum in a fixed order over the fp32 distances."""
    _, _, s1 = nearest_neighbor(recon_points, gt_points)
    _, _, s2 = nearest_neighbor(gt_points, recon_points)
    return 0.5 * (s1 / len(gt_points) + s2 / len(recon_points))


# ---- the exported mesh: orientation, vertex compaction, topology (reference processing/generate_mesh.py:107-124) ------------------
@on_device_of
def orient_interface(vertices, tetrahedra, facets, nfacets, labels, face_ids, orient=True, return_exact_used=False):
    """The interface facets facets[face_ids] as faces int32 [K, 3] on the GPU, each wound so that its normal points away from its inside
    cell (labels[c] == 0; cell -1 = the infinite cell, outside), by the EXACT sign of det[b - a, c - a, d - a] (dgnn_orient_interface; the
    rule and its flat-cell cases are in include/dgnn_hip.h).  orient=False keeps the stored winding (the facets are still checked).
    -> (faces, n_undetermined) (+ whether the exact stage ran for some facet with return_exact_used).  DgnnError for malformed input."""
    dev = _dev_of(labels, face_ids, vertices)
    v, tets, fac, nfac = _scene(dev, vertices, tetrahedra, facets, nfacets)
    lab = _on(labels, dev, torch.int32).reshape(-1)
    ids = _on(face_ids, dev, torch.int32).reshape(-1)
    if lab.numel() != tets.size(0):
        raise ValueError("%d labels for %d cells" % (lab.numel(), tets.size(0)))
    k = ids.numel()
    faces = _empty(dev, torch.int32, k, 3)
    und = torch.zeros(1, dtype=torch.int64, device=dev)
    used = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = _scratch(dev, lib().dgnn_orient_interface_scratch_bytes())
    check(lib().dgnn_orient_interface(ptr(v), v.size(0), ptr(tets), tets.size(0), ptr(fac), ptr(nfac), fac.size(0), ptr(lab), ptr(ids), k,
                                      int(bool(orient)), ptr(faces), ptr(und), ptr(used), ptr(scratch), stream_ptr()), "dgnn_orient_interface")
    return (faces, int(und.item()), bool(used.item())) if return_exact_used else (faces, int(und.item()))


@on_device_of
def compact_vertices(faces, n_vertices):
    """The vertices that `faces` references, in ascending id, and the faces renumbered onto them (dgnn_compact_vertices, which
    compacts with dgnn_compact_i32).  -> (faces int32 [K, 3], kept vertex ids int32 [M]) on the GPU."""
    dev = _dev_of(faces)
    f = _on(faces, dev, torch.int32, 3)
    nv, k = int(n_vertices), f.size(0)
    out = _empty(dev, torch.int32, k, 3)
    kept = torch.empty(max(nv, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = _scratch(dev, lib().dgnn_compact_vertices_scratch_bytes(nv))
    check(lib().dgnn_compact_vertices(ptr(f), k, nv, ptr(out), ptr(kept), ptr(cnt), ptr(scratch), stream_ptr()), "dgnn_compact_vertices")
    return out, kept[:int(cnt.item())]


MESH_TOPOLOGY_KEYS = ("n_edges", "boundary_edges", "nonmanifold_edges", "nonmanifold_vertices", "winding_mismatch_edges")


@on_device_of
def mesh_topology(faces, n_vertices):
    """Edge and vertex counts of a triangle mesh (dgnn_mesh_topology): dict of MESH_TOPOLOGY_KEYS -> int, plus
    watertight = boundary_edges == nonmanifold_edges == nonmanifold_vertices == 0 (Open3D's is_watertight without its self-intersection
    test; an empty mesh is not watertight).  DgnnError for ids out of range or a face with a repeated vertex."""
    dev = _dev_of(faces)
    f = _on(faces, dev, torch.int32, 3)
    nv, k = int(n_vertices), f.size(0)
    counts = torch.zeros(5, dtype=torch.int64, device=dev)
    scratch = _scratch(dev, lib().dgnn_mesh_topology_scratch_bytes(k, nv))
    check(lib().dgnn_mesh_topology(ptr(f), k, nv, ptr(counts), ptr(scratch), stream_ptr()), "dgnn_mesh_topology")
    out = _stats_dict(MESH_TOPOLOGY_KEYS, counts)
    out["watertight"] = int(k > 0 and out["boundary_edges"] == 0 and out["nonmanifold_edges"] == 0 and out["nonmanifold_vertices"] == 0)
    return out


# ---- connected components of a triangle mesh (csrc/meshcomp.hip; the reference: trimesh split / body_count) --------------------------
@on_device_of
def mesh_components(faces, n_vertices):
    """Connected components of a triangle mesh (dgnn_mesh_components): faces that share an undirected edge are connected, however many
    faces meet on it; a shared vertex alone does not connect.  -> (comp int32 [F] on the GPU, K): components 0..K-1 numbered in ascending
    order of their smallest face id, the same on every run.  DgnnError for ids out of range or a face with a repeated vertex."""
    dev = _dev_of(faces)
    f = _on(faces, dev, torch.int32, 3)
    nv, k = int(n_vertices), f.size(0)
    comp = _empty(dev, torch.int32, k)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = _scratch(dev, lib().dgnn_mesh_components_scratch_bytes(k), or_one=True)
    check(lib().dgnn_mesh_components(ptr(f), k, nv, ptr(comp), ptr(cnt), ptr(scratch), stream_ptr()), "dgnn_mesh_components")
    return comp, int(cnt.item())


@on_device_of
def mesh_component_measures(vertices, faces, comp, K):
    """Per component of `comp` (mesh_components): {"n_faces": int64 [K], "area": fp64 [K], "signed_volume": fp64 [K]} on the GPU
    (dgnn_mesh_component_measures).  signed_volume = sum of v0 . (v1 x v2) / 6 over the component's faces in their stored winding: the
    enclosed volume of a closed component wound outward, its negative when wound inward.  Sums run in a fixed order (include/dgnn_hip.h):
    reruns are bit-identical.  DgnnError for a vertex or component id out of range."""
    dev = _dev_of(comp, faces, vertices)
    v = _on(vertices, dev, torch.float64, 3)
    f = _on(faces, dev, torch.int32, 3)
    c = _on(comp, dev, torch.int32).reshape(-1)
    nf, k = f.size(0), int(K)
    if c.numel() != nf:
        raise ValueError("%d component ids for %d faces" % (c.numel(), nf))
    n, area, vol = _zeros(dev, torch.int64, k), _zeros(dev, torch.float64, k), _zeros(dev, torch.float64, k)
    scratch = _scratch(dev, lib().dgnn_mesh_component_measures_scratch_bytes(nf, k), or_one=True)
    check(lib().dgnn_mesh_component_measures(ptr(v), v.size(0), ptr(f), nf, ptr(c), k, ptr(n), ptr(area), ptr(vol), ptr(scratch), stream_ptr()),
          "dgnn_mesh_component_measures")
    return {"n_faces": n, "area": area, "signed_volume": vol}


@on_device_of
def filter_components(faces, comp, counts, largest=False, min_faces=None):
    """The faces of the components a rule keeps (dgnn_mesh_component_keep, then dgnn_compact_i32: face order preserved): `largest` = the
    one component with the most faces (a tie goes to the smaller component id), `min_faces=n` = every component with at least n faces.
    counts: the "n_faces" of mesh_component_measures.  -> (faces int32 [n_kept, 3], keep bool [F], n_kept), tensors on the GPU."""
    if bool(largest) == (min_faces is not None):
        raise ValueError("filter_components: give either largest=True or min_faces=n")
    if min_faces is not None and int(min_faces) < 1:
        raise ValueError("filter_components: min_faces=%r, expected an int >= 1" % (min_faces,))
    dev = _dev_of(comp, faces, counts)
    f = _on(faces, dev, torch.int32, 3)
    c = _on(comp, dev, torch.int32).reshape(-1)
    cnt = _on(counts, dev, torch.int64).reshape(-1)
    nf = f.size(0)
    if c.numel() != nf:
        raise ValueError("%d component ids for %d faces" % (c.numel(), nf))
    keep = _zeros(dev, torch.int32, nf)
    n_kept = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = _scratch(dev, lib().dgnn_mesh_component_keep_scratch_bytes())
    check(lib().dgnn_mesh_component_keep(ptr(c), nf, ptr(cnt), cnt.numel(), 0 if largest else 1, 1 if largest else int(min_faces), ptr(keep),
                                         ptr(n_kept), ptr(scratch), stream_ptr()), "dgnn_mesh_component_keep")
    ids = torch.empty(max(nf, 1), dtype=torch.int32, device=dev)
    got = torch.zeros(1, dtype=torch.int32, device=dev)
    cscratch = torch.empty(int(lib().dgnn_compact_scratch_elems(nf)), dtype=torch.int32, device=dev)
    check(lib().dgnn_compact_i32(None, ptr(keep), 0, nf, ptr(ids), ptr(got), ptr(cscratch), stream_ptr()), "dgnn_compact_i32")
    m = int(n_kept.item())
    if int(got.item()) != m:
        raise DgnnError("filter_components: %d faces flagged, %d compacted" % (m, int(got.item())))
    return f[ids[:m].long()], keep.bool(), m


# ---- the scene front end: adjacency, cell geometry, vertex-ray visibility (csrc/scenefeat.hip) ---------------------------
@on_device_of
def tet_neighbors(facets, nfacets, tetrahedra):
    """neighbors int32 [T, 4] on the GPU (dgnn_tet_neighbors): slot k = the cell across the facet opposite vertex k of the tet, -1 = the
    infinite cell; facets int [F, 3], nfacets int [F, 2], tetrahedra int [T, 4] of a `_3dt.npz`.  DgnnError for ids out of range and
    for a facet that is not a face of a cell nfacets names for it."""
    dev = _dev_of(tetrahedra, facets, nfacets)
    _, tets, fac, nfac = _scene(dev, None, tetrahedra, facets, nfacets)
    t = tets.size(0)
    nbr = _empty(dev, torch.int32, t, 4)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = _scratch(dev, lib().dgnn_tet_neighbors_scratch_bytes())
    check(lib().dgnn_tet_neighbors(ptr(tets), t, ptr(fac), ptr(nfac), fac.size(0), ptr(nbr), ptr(bad), ptr(scratch), stream_ptr()), "dgnn_tet_neighbors")
    if int(bad.item()):
        raise DgnnError("tet_neighbors: %d (facet, cell) pairs whose facet is not a face of the cell nfacets names" % int(bad.item()))
    return nbr


@on_device_of
def cell_geometry(vertices, tetrahedra):
    """The `_cgeom` columns of the finite cells (dgnn_cell_geometry; the expressions are in include/dgnn_hip.h): dict of "radius"
    (circumradius, +inf for a flat cell), "vol", "longest_edge", "shortest_edge" fp64 [T] on the GPU, "n_flat" int, and "sum_longest",
    "sum_shortest" floats: the two column sums in a fixed order, from which the loader's mean_edge over n cells is
    (sum_longest + sum_shortest) / (2 n).  DgnnError for a vertex id out of range."""
    dev = _dev_of(vertices, tetrahedra)
    v = _on(vertices, dev, torch.float64, 3)
    tets = _on(tetrahedra, dev, torch.int32, 4)
    t = tets.size(0)
    cols = [_empty(dev, torch.float64, t) for _ in range(4)]
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    flat = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = _scratch(dev, lib().dgnn_cell_geometry_scratch_bytes(t))
    check(lib().dgnn_cell_geometry(ptr(v), v.size(0), ptr(tets), t, ptr(cols[0]), ptr(cols[1]), ptr(cols[2]), ptr(cols[3]), ptr(sums), ptr(flat),
                                   ptr(scratch), stream_ptr()), "dgnn_cell_geometry")
    s = sums.cpu()
    return {"radius": cols[0], "vol": cols[1], "longest_edge": cols[2], "shortest_edge": cols[3], "n_flat": int(flat.item()),
            "sum_longest": float(s[0]), "sum_shortest": float(s[1])}


FGEOM_KEYS = ("area", "cos_own", "cos_neighbor", "beta")          # the keys of `_fgeom.npz`, in the file's order


@on_device_of
def cell_circumspheres(vertices, tetrahedra):
    """The circumsphere of every finite cell (dgnn_cell_circumspheres; §23's expressions): dict of "centre" fp64 [T, 3] and
    "radius" fp64 [T] on the GPU, "n_flat" int: the cells with det == 0, whose radius is inf or NaN, and "records": the [T, 4] array
    (o.x, o.y, o.z, R) that the two are views of and that facet_geometry reads in place.  DgnnError for a vertex id out of range."""
    dev = _dev_of(vertices, tetrahedra)
    v = _on(vertices, dev, torch.float64, 3)
    tets = _on(tetrahedra, dev, torch.int32, 4)
    t = tets.size(0)
    rec = _empty(dev, torch.float64, t, 4)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    scratch = _scratch(dev, lib().dgnn_cell_circumspheres_scratch_bytes())
    check(lib().dgnn_cell_circumspheres(ptr(v), v.size(0), ptr(tets), t, ptr(rec), ptr(stats), ptr(scratch), stream_ptr()), "dgnn_cell_circumspheres")
    return {"centre": rec[:, :3], "radius": rec[:, 3], "n_flat": int(stats[3].item()), "records": rec}


@on_device_of
def facet_geometry(vertices, tetrahedra, facets, nfacets, spheres=None):
    """The `_fgeom` columns of the finite cells from the arrays of `<scene>_3dt.npz` (dgnn_facet_geometry; the definition is in
    include/dgnn_hip.h and DESIGN §32): row 4 t + k belongs to the facet of tet t opposite its vertex k and holds the facet's "area", the
    circumsphere cosine of §23 on the tet's side ("cos_own") and on the other side ("cos_neighbor"; 1.0 when that is the infinite cell) and
    "beta" = 1 - min of the two.  vertices fp64 [V, 3], tetrahedra int [T, 4], facets int [F, 3], nfacets int [F, 2].  spheres: the dict of
    cell_circumspheres for these cells (computed here when None).
    -> dict of the four FGEOM_KEYS tensors, fp64 [4 T] on the GPU (0 in a row that no facet names), and "stats": {"rows" (rows written),
    "hull_rows" (those whose neighbour is the infinite cell), "neutral_sides", "n_flat"}.  DgnnError for an id out of range and for a facet
    that is not a face of a cell its nfacets row names."""
    dev = _dev_of(vertices, tetrahedra, facets, nfacets)
    v, tets, fac, nfac = _scene(dev, vertices, tetrahedra, facets, nfacets)
    t = tets.size(0)
    rec = None
    if spheres is not None:
        if not isinstance(spheres, dict) or "records" not in spheres or "n_flat" not in spheres:
            raise ValueError("facet_geometry: spheres must be the dict cell_circumspheres returned (its \"records\" and \"n_flat\")")
        rec = _on(spheres["records"], dev, torch.float64, 4)
        if rec.size(0) != t:
            raise ValueError("spheres of %d cells for %d tetrahedra" % (rec.size(0), t))
        if rec.data_ptr() % 32:          # a view into a larger tensor: the kernel loads whole 32-byte records
            rec = rec.clone()
    out = _empty(dev, torch.float64, 4, 4 * t)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    scratch = _scratch(dev, lib().dgnn_facet_geometry_scratch_bytes(t))
    check(lib().dgnn_facet_geometry(ptr(v), v.size(0), ptr(tets), t, ptr(fac), ptr(nfac), fac.size(0), ptr(rec), ptr(out), ptr(stats), ptr(scratch),
                                    stream_ptr()), "dgnn_facet_geometry")
    s = [int(x) for x in stats.cpu()]
    res = {k: out[i] for i, k in enumerate(FGEOM_KEYS)}
    res["stats"] = {"rows": s[0], "hull_rows": s[1], "neutral_sides": s[2], "n_flat": int(spheres["n_flat"]) if spheres is not None else s[3]}
    return res


@on_device_of
def vertex_incidence(tetrahedra, n_vertices):
    """(rowptr int32 [V + 1], entries int32 [4 T]) on the GPU (dgnn_vertex_incidence): row v holds 4 t + k for every corner
    tetrahedra[t][k] == v.  The order inside a row is not specified.  DgnnError for a vertex id out of range."""
    dev = _dev_of(tetrahedra)
    tets = _on(tetrahedra, dev, torch.int32, 4)
    t, nv = tets.size(0), int(n_vertices)
    rowptr = torch.zeros(nv + 1, dtype=torch.int32, device=dev)
    entries = _empty(dev, torch.int32, 4 * t)
    scratch = _scratch(dev, lib().dgnn_vertex_incidence_scratch_bytes(nv))
    check(lib().dgnn_vertex_incidence(ptr(tets), t, nv, ptr(rowptr), ptr(entries), ptr(scratch), stream_ptr()), "dgnn_vertex_incidence")
    return rowptr, entries


RAY_SIDES = ("outside", "inside")
RAY_STATS = ("used", "duplicates", "degenerate", "no_outside", "no_inside", "exact_used")


@on_device_of
def vertex_ray_features(vertices, tetrahedra, ray_vertex, sensors, unique=True, incidence=None):
    """The vertex-ray visibility aggregates (dgnn_vertex_rays; cell choice, tie rule and the distance are in include/dgnn_hip.h): ray r
    runs from vertices[ray_vertex[r]] towards sensors[r] (fp64 [R, 3]); with `unique` only the lowest-index ray of a vertex is used.
    incidence: the pair of vertex_incidence (built here when None).  -> dict of tensors on the GPU:
      "ray_tet", "ray_slot" int32 [R, 2], "ray_dist" fp64 [R, 2]: the chosen cell per side (column 0 outside, 1 inside; -1 / 0.0 = none);
      "<side>_tet_count" int32 [T], "<side>_tet_{min,max,sum}" fp64 [T], "<side>_slot_count" int32 [T, 4], "<side>_slot_{min,max,sum}"
      fp64 [T, 4] for <side> in RAY_SIDES; "stats": dict of RAY_STATS -> int.
    DgnnError for ids out of range and coordinates outside the exact predicate's range."""
    dev, v, tets, rv, s, rowptr, entries = _ray_inputs(vertices, tetrahedra, ray_vertex, sensors, incidence)
    t, r, nv = tets.size(0), rv.numel(), v.size(0)
    ray_tet, ray_slot, ray_dist = _empty(dev, torch.int32, r, 2), _empty(dev, torch.int32, r, 2), _empty(dev, torch.float64, r, 2)
    tet_count, tet_stat = _empty(dev, torch.int32, 2, t), _empty(dev, torch.float64, 2, 3, t)
    slot_count, slot_stat = _empty(dev, torch.int32, 2, t, 4), _empty(dev, torch.float64, 2, 3, t, 4)
    stats = torch.zeros(len(RAY_STATS), dtype=torch.int64, device=dev)
    scratch = _scratch(dev, lib().dgnn_vertex_rays_scratch_bytes(r, t, nv), or_one=True)
    check(lib().dgnn_vertex_rays(ptr(v), nv, ptr(tets), t, ptr(rowptr), ptr(entries), ptr(rv), ptr(s), r, int(bool(unique)), ptr(ray_tet), ptr(ray_slot),
                                 ptr(ray_dist), ptr(tet_count), ptr(tet_stat), ptr(slot_count), ptr(slot_stat), ptr(stats), ptr(scratch), stream_ptr()),
          "dgnn_vertex_rays")
    out = {"ray_tet": ray_tet, "ray_slot": ray_slot, "ray_dist": ray_dist, "stats": _stats_dict(RAY_STATS, stats)}
    _side_columns(out, "tet", tet_count, tet_stat)
    _side_columns(out, "slot", slot_count, slot_stat)
    return out


# ---- the facet-ray walk: every ray through all the cells it crosses (csrc/raywalk.hip) -------------------------------------
WALK_STATUS = ("none", "sensor", "hull", "depth", "stuck", "capped")
WALK_STATS = ("used", "skipped", "perturbed", "exact_used", "degenerate") + WALK_STATUS + ("records", "longest")
WALK_RECORD_KEYS = ("ray", "side", "step", "cell", "slot", "first", "second")
WALK_DEFAULT_RECORDS = 1 << 22          # records staged at a time: 48 bytes each plus the sort's histograms


@on_device_of
def ray_walk(vertices, tetrahedra, neighbors, ray_vertex, sensors, unique=True, outside_depth=0, inside_depth=1, max_records=None, incidence=None,
             return_records=False):
    """Walks every ray through the triangulation (dgnn_ray_walk; the rule -- the perturbed side test, the start cells, the steps and the
    ends -- is in include/dgnn_hip.h).  Ray r runs from vertices[ray_vertex[r]] to sensors[r] (fp64 [R, 3]); side `outside` walks towards
    the sensor, `inside` away from it, through neighbors int [T, 4] (ops.tet_neighbors: -1 = the infinite cell).  The start cell is the
    vertex family's and is not recorded; outside_depth / inside_depth end a walk after that many recorded cells (0: no limit).
    max_records bounds the staged record stream (None: WALK_DEFAULT_RECORDS, or T + 1 when that is more -- no walk is longer); no result
    depends on it.  incidence: the pair of vertex_incidence (built here when None).  -> dict of tensors on the GPU, <side> in RAY_SIDES:
      "<side>_cell_count" int32 [T], "<side>_cell_{first,second}_{min,max,sum}" fp64 [T]: over the recorded crossings of the cell, the
      distance from the ray's vertex to where it enters (first) and leaves (second; in the sensor's cell the sensor's distance);
      "<side>_slot_count" int32 [T, 4], "<side>_slot_{min,max,sum}" fp64 [T, 4]: per facet (c, k) of the cell the ray leaves;
      "ray_status" int32 [R, 2] (index into WALK_STATUS), "ray_cells" int32 [R, 2]; "stats": dict of WALK_STATS -> int;
      with return_records "records": dict of WALK_RECORD_KEYS -> tensor, ascending (ray, side, step) (the walk then runs twice).
    DgnnError for ids out of range, coordinates outside the exact predicate's range and a max_records below the longest walk."""
    dev, v, tets, rv, s, rowptr, entries = _ray_inputs(vertices, tetrahedra, ray_vertex, sensors, incidence)
    nbr = _on(neighbors, dev, torch.int32, 4)
    t, r, nv = tets.size(0), rv.numel(), v.size(0)
    if nbr.size(0) != t:
        raise ValueError("%d neighbour rows for %d tets" % (nbr.size(0), t))
    m = max(WALK_DEFAULT_RECORDS, t + 1) if max_records is None else int(max_records)
    scratch = _scratch(dev, lib().dgnn_ray_walk_scratch_bytes(r, t, nv, m), "ray_walk: %d rays, %d tets, max_records %d exceed the int32 indexing" % (r, t, m))

    def run(capacity):
        status, cells = _empty(dev, torch.int32, r, 2), _empty(dev, torch.int32, r, 2)
        cell_count, cell_stat = _empty(dev, torch.int32, 2, t), _empty(dev, torch.float64, 2, 6, t)
        slot_count, slot_stat = _empty(dev, torch.int32, 2, t, 4), _empty(dev, torch.float64, 2, 3, t, 4)
        stats = torch.zeros(len(WALK_STATS), dtype=torch.int64, device=dev)
        ids, dist = _empty(dev, torch.int32, 5, capacity), _empty(dev, torch.float64, 2, capacity)
        check(lib().dgnn_ray_walk(ptr(v), nv, ptr(tets), t, ptr(nbr), ptr(rowptr), ptr(entries), ptr(rv), ptr(s), r, int(bool(unique)), int(outside_depth),
                                  int(inside_depth), m, ptr(status), ptr(cells), ptr(cell_count), ptr(cell_stat), ptr(slot_count), ptr(slot_stat),
                                  ptr(stats), capacity, ptr(ids), ptr(dist), ptr(scratch), stream_ptr()), "dgnn_ray_walk")
        out = {"ray_status": status, "ray_cells": cells, "stats": _stats_dict(WALK_STATS, stats)}
        _side_columns(out, "cell", cell_count, cell_stat, ("first_", "second_"))
        _side_columns(out, "slot", slot_count, slot_stat)
        if capacity:
            out["records"] = dict(zip(WALK_RECORD_KEYS, list(ids) + list(dist)))
        return out

    out = run(0)
    if return_records:          # the stream's length is known only after a walk
        n = out["stats"]["records"]
        out = run(n) if n else dict(out, records=dict(zip(WALK_RECORD_KEYS, list(_empty(dev, torch.int32, 5, 0)) + list(_empty(dev, torch.float64, 2, 0)))))
    return out


# ---- occupancy of any triangle mesh and the evaluation-sample generators (csrc/meshcontains.hip; reference utils/libmesh) ----------
def _check_value(code, what):
    """`check`, with the library's "bad input" status as the ValueError a Python caller expects for bad data"""
    if code == -1:
        raise ValueError("%s: %s" % (what, lib().dgnn_last_error_string().decode()))
    check(code, what)


def _points64(points, dev):
    t = torch.as_tensor(points)
    if t.dtype not in (torch.float16, torch.float32, torch.float64):
        raise ValueError("points must be fp16, fp32 or fp64, got %s" % t.dtype)
    return _on(t, dev, torch.float64, 3)     # every fp16 / fp32 value is an fp64 value: exact


def _planned_entries(dev, what, plan):
    """The candidate grid's entry list, sized by its planning call: plan(byref(n_entries)) -> status.  -> (entries int32, their number of
    places, at least one)."""
    n_entries = C.c_int64(0)
    _check_value(plan(C.byref(n_entries)), what)
    cap = max(int(n_entries.value), 1)
    return torch.empty(cap, dtype=torch.int32, device=dev), cap


def _mesh_contains_entries(dev, v, f, R, max_entries, scratch):
    return _planned_entries(dev, "dgnn_mesh_contains_plan", lambda n: lib().dgnn_mesh_contains_plan(
        ptr(v), v.size(0), ptr(f), f.size(0), R, int(max_entries), C.byref(C.c_int32(0)), n, ptr(scratch), stream_ptr()))


@on_device_of
def mesh_contains(vertices, faces, points, hash_resolution=512, max_entries=2 ** 30):
    """check_mesh_contains(mesh, points, hash_resolution) of the reference's utils/libmesh on the device (dgnn_mesh_contains; the
    arithmetic is in include/dgnn_hip.h): vertices [V, 3] and points [n, 3] (fp16 / fp32 / fp64, tensor or ndarray) are promoted to fp64,
    faces int [F, 3].  -> (contains bool [n] on the GPU, n_disagree: the points whose two ray parities differ, for which the reference
    prints its warning).  max_entries caps the (triangle, cell) entries of the candidate grid, which is coarsened to fit; the answer does
    not depend on it.  ValueError for a mesh without faces or without extent on an axis, a face id out of range or a non-finite
    referenced vertex; DgnnError for hash_resolution above 4096 or max_entries below the number of faces."""
    dev = _dev_of(points, vertices, faces)
    v = _on(vertices, dev, torch.float64, 3)
    f = _on(faces, dev, torch.int32, 3)
    pts = _points64(points, dev)
    nv, nf, n, R = v.size(0), f.size(0), pts.size(0), int(hash_resolution)
    if nf == 0:
        raise ValueError("mesh_contains: a mesh without faces")
    out = _empty(dev, torch.bool, n)
    if n == 0:
        return out, 0
    scratch = _scratch(dev, lib().dgnn_mesh_contains_scratch_bytes(nv, nf, R))
    entries, cap = _mesh_contains_entries(dev, v, f, R, max_entries, scratch)
    dis = torch.zeros(1, dtype=torch.int64, device=dev)
    _check_value(lib().dgnn_mesh_contains(ptr(v), nv, ptr(f), nf, R, int(max_entries), ptr(pts), n, ptr(out), ptr(dis), ptr(entries), cap,
                                          ptr(scratch), stream_ptr()), "dgnn_mesh_contains")
    return out, int(dis.item())


def mesh_occupancy_iou(vertices, faces, points, occ_gt):
    """IoU of the mesh's occupancy at `points` (mesh_contains) with the ground-truth occupancies occ_gt [n] (non-zero = inside), as
    compute_iou computes it (the integer counts of iou_counts, float32 ratio; nan for an empty union): the reference's `iou` metric
    (processing/generate_mesh.py:139-141) for a mesh from anywhere.  -> (iou float, occupancy bool [n] on the GPU, |A n B|, |A u B|)."""
    import numpy as np

    occ, n_disagree = mesh_contains(vertices, faces, points)
    if n_disagree:
        print("Warning: contains1 != contains2 for some points.")
    cells = occ.to(torch.int32) - 1                                  # "cell 0, labelled inside" or "no cell"
    _, inter, union = iou_counts(cells, torch.zeros(1, dtype=torch.int32, device=occ.device), occ_gt)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = float(np.float32(inter) / np.float32(union))
    return iou, occ, inter, union


@on_device_of
def face_normals(vertices, faces):
    """Unit normals fp64 [F, 3] on the GPU of the faces (v0, v1, v2): (v1 - v0) x (v2 - v0), normalised; zeros for a face without area
    (dgnn_face_normals).  ValueError for a face id out of range."""
    dev = _dev_of(vertices, faces)
    v = _on(vertices, dev, torch.float64, 3)
    f = _on(faces, dev, torch.int32, 3)
    nf = f.size(0)
    out = _empty(dev, torch.float64, nf, 3)
    scratch = _scratch(dev, 256)
    _check_value(lib().dgnn_face_normals(ptr(v), v.size(0), ptr(f), nf, ptr(out), ptr(scratch), stream_ptr()), "dgnn_face_normals")
    return out


def _seed64(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def box_points(n, boxsize, seed=0, device=None):
    """n points fp64 [n, 3] on the GPU, uniform in the cube of edge `boxsize` about the origin: boxsize * (u - 0.5) with u in [0, 1) from
    mm_hash(seed, .) (dgnn_box_points; include/dgnn_hip.h)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    n = int(n)
    with torch.cuda.device(dev):
        out = _empty(dev, torch.float64, n, 3)
        check(lib().dgnn_box_points(n, float(boxsize), _seed64(seed), ptr(out), stream_ptr()), "dgnn_box_points")
    return out


@on_device_of
def jitter_points(points64, sigma, seed=0):
    """points64 (fp64 [n, 3]) + sigma * N(0, 1) per coordinate, Box-Muller in fp64 on two mm_hash draws (dgnn_jitter_points) -> a new
    fp64 tensor on the GPU."""
    dev = _dev_of(points64)
    p = _on(points64, dev, torch.float64, 3)
    n = p.size(0)
    out = _empty(dev, torch.float64, n, 3)
    check(lib().dgnn_jitter_points(ptr(p), n, float(sigma), _seed64(seed), ptr(out), stream_ptr()), "dgnn_jitter_points")
    return out


# ---- ground-truth cell labels: the share of each tet inside a closed mesh (csrc/meshcontains.hip) -----------------------
@on_device_of
def tet_sample_points(vertices, tetrahedra, n_samples, seed=0, tet_offset=0):
    """n_samples points in every tet, uniform by volume, fp64 [T * n_samples, 3] on the GPU (dgnn_tet_sample_points; the draws, the fold
    onto the tet and the operation order are in include/dgnn_hip.h): row t * n_samples + j is sample j of tet t, the very point
    cell_labels tests.  tet_offset shifts the counters, so a chunk [a, b) of the tets with tet_offset=a gives rows of the whole call.
    ValueError for n_samples < 1, DgnnError for a tet id out of range."""
    dev = _dev_of(vertices, tetrahedra)
    v = _on(vertices, dev, torch.float64, 3)
    tets = _on(tetrahedra, dev, torch.int32, 4)
    k, t = int(n_samples), tets.size(0)
    if k < 1:
        raise ValueError("tet_sample_points: n_samples %d < 1" % k)
    out = _empty(dev, torch.float64, t * k, 3)
    scratch = _scratch(dev, lib().dgnn_tet_sample_points_scratch_bytes())
    check(lib().dgnn_tet_sample_points(ptr(v), v.size(0), ptr(tets), t, k, _seed64(seed), _seed64(tet_offset), ptr(out), ptr(scratch), stream_ptr()),
          "dgnn_tet_sample_points")
    return out


@on_device_of
def cell_labels(mesh_vertices, mesh_faces, vertices, tetrahedra, n_samples=100, seed=0, tet_offset=0, hash_resolution=512, max_entries=2 ** 30):
    """The share of every tet (vertices [V, 3], tetrahedra int [T, 4]) inside the closed mesh (mesh_vertices [M, 3], mesh_faces int [F, 3]):
    n_samples points per tet, each tested as mesh_contains tests it, in one fused kernel that keeps the samples in registers
    (dgnn_cell_labels; definitions in include/dgnn_hip.h).  -> dict: "count" int32 [T] (the inside samples), "inside_perc" = count /
    n_samples and "outside_perc" = (n_samples - count) / n_samples, fp64 [T], all on the GPU; "n_samples"; "n_disagree": the samples whose
    two ray parities differ (counted as outside).  The result does not depend on max_entries; tet_offset as in tet_sample_points.
    ValueError for n_samples < 1 and for what mesh_contains refuses in a mesh (no faces, no extent, a face id out of range, a non-finite
    referenced vertex); DgnnError for a tet id out of range."""
    dev = _dev_of(vertices, tetrahedra, mesh_vertices, mesh_faces)
    mv = _on(mesh_vertices, dev, torch.float64, 3)
    mf = _on(mesh_faces, dev, torch.int32, 3)
    v = _on(vertices, dev, torch.float64, 3)
    tets = _on(tetrahedra, dev, torch.int32, 4)
    k, t, nv, nf, R = int(n_samples), tets.size(0), mv.size(0), mf.size(0), int(hash_resolution)
    if k < 1:
        raise ValueError("cell_labels: n_samples %d < 1" % k)
    if nf == 0:
        raise ValueError("cell_labels: a mesh without faces")
    scratch = _scratch(dev, lib().dgnn_cell_labels_scratch_bytes(nv, nf, R))
    entries, cap = _mesh_contains_entries(dev, mv, mf, R, max_entries, scratch)
    count =_empty(dev, torch.int32, t)
    dis = torch.zeros(1, dtype=torch.int64, device=dev)
    # the mesh passed the plan above: what is refused from here on is the tets' ids
    check(lib().dgnn_cell_labels(ptr(mv), nv, ptr(mf), nf, R, int(max_entries), ptr(entries), cap, ptr(v), v.size(0), ptr(tets), t, k, _seed64(seed),
                                 _seed64(tet_offset), ptr(count), ptr(dis), ptr(scratch), stream_ptr()), "dgnn_cell_labels")
    kd = torch.full_like(count, k, dtype=torch.float64)          # a tensor divisor: a true fp64 division (a Python scalar would be multiplied by 1 / k)
    return {"count": count, "inside_perc": count.double() / kd, "outside_perc": (k - count).double() / kd, "n_samples": k,
            "n_disagree": int(dis.item())}


# ---- first-hit ray casting on a triangle mesh (csrc/raycast.hip) ---------------------------------------------------------
RAY_HIT_STATS = ("hits", "skipped", "degenerate", "exact_used")


def default_grid_resolution(n_faces):
    """The grid resolution ray_first_hit takes when none is given: sqrt(n_faces) / 2 cells along the longest axis, within [1, 256] (the sweep
    behind it is profiles/scan_mesh.md).  The answer does not depend on it."""
    return max(1, min(256, int(round(0.5 * float(n_faces) ** 0.5))))


@on_device_of
def ray_first_hit(vertices, faces, origins, aims, t_min=0.0, grid_resolution=None, return_stats=False):
    """The first face of the mesh (vertices [V, 3], faces int [F, 3]) that each ray from origins[r] through aims[r] (fp16 / fp32 / fp64 [n, 3],
    promoted to fp64) crosses beyond t_min, the aim being at t = 1 (dgnn_ray_first_hit; the exact crossing rule, the parameter and the tie
    rule are in include/dgnn_hip.h).  -> (face int32 [n], -1 = none; t fp64 [n], 0 where none; point fp64 [n, 3] = origin + t (aim - origin),
    zeros where none), all on the GPU; with return_stats also a dict of RAY_HIT_STATS -> int.  grid_resolution (None: default_grid_resolution
    of the face count) sizes the candidate grid; the answer does not depend on it.  ValueError for a mesh without faces, a face id out of
    range, a non-finite referenced vertex, origin or aim and a negative t_min; DgnnError for a coordinate magnitude outside [2^-300, 2^300]
    and a grid_resolution outside [1, 1024]."""
    dev = _dev_of(origins, aims, vertices, faces)
    v = _on(vertices, dev, torch.float64, 3)
    f = _on(faces, dev, torch.int32, 3)
    o, g = _points64(origins, dev), _points64(aims, dev)
    if o.size(0) != g.size(0):
        raise ValueError("ray_first_hit: %d origins for %d aims" % (o.size(0), g.size(0)))
    nv, nf, n = v.size(0), f.size(0), o.size(0)
    if nf == 0:
        raise ValueError("ray_first_hit: a mesh without faces")
    R = default_grid_resolution(nf) if grid_resolution is None else int(grid_resolution)
    scratch = _scratch(dev, lib().dgnn_ray_first_hit_scratch_bytes(nf, R))
    entries, cap = _planned_entries(dev, "dgnn_ray_first_hit_plan", lambda n_entries: lib().dgnn_ray_first_hit_plan(
        ptr(v), nv, ptr(f), nf, R, n_entries, None, ptr(scratch), stream_ptr()))
    face, t, point = _empty(dev, torch.int32, n), _empty(dev, torch.float64, n), _empty(dev, torch.float64, n, 3)
    stats = torch.zeros(len(RAY_HIT_STATS), dtype=torch.int64, device=dev)
    _check_value(lib().dgnn_ray_first_hit(ptr(v), nv, ptr(f), nf, R, ptr(o), ptr(g), n, float(t_min), ptr(face), ptr(t), ptr(point), ptr(stats), ptr(entries),
                                          cap, ptr(scratch), stream_ptr()), "dgnn_ray_first_hit")
    if return_stats:
        return face, t, point, _stats_dict(RAY_HIT_STATS, stats)
    return face, t, point


# ---- point-to-mesh distance and the surface metrics built on it (csrc/meshdist.hip) ---------------------------------------
MESH_DISTANCE_STATS = ("entries", "max_shells", "shells", "faces_evaluated")


def _point_mesh_d2(vertices, faces, points, grid_resolution, what):
    dev = _dev_of(points, vertices, faces)
    v = _on(vertices, dev, torch.float64, 3)
    f = _on(faces, dev, torch.int32, 3)
    pts = _points64(points, dev)
    nv, nf, n = v.size(0), f.size(0), pts.size(0)
    if nf == 0:
        raise ValueError("%s: a mesh without faces" % what)
    R = default_grid_resolution(nf) if grid_resolution is None else int(grid_resolution)
    scratch = _scratch(dev, lib().dgnn_point_mesh_distance_scratch_bytes(nf, R))
    entries, cap = None, 0
    if R != 0:          # (a resolution the library refuses is refused by the planning call)
        entries, cap = _planned_entries(dev, "dgnn_point_mesh_distance_plan", lambda n_entries: lib().dgnn_point_mesh_distance_plan(
            ptr(v), nv, ptr(f), nf, R, n_entries, ptr(scratch), stream_ptr()))
    d2, dist, face = _empty(dev, torch.float64, n), _empty(dev, torch.float64, n), _empty(dev, torch.int32, n)
    closest, region = _empty(dev, torch.float64, n, 3), _empty(dev, torch.uint8, n)
    stats = torch.zeros(len(MESH_DISTANCE_STATS), dtype=torch.int64, device=dev)
    _check_value(lib().dgnn_point_mesh_distance(ptr(v), nv, ptr(f), nf, R, ptr(pts), n, ptr(d2), ptr(dist), ptr(face), ptr(closest), ptr(region), ptr(stats),
                                                ptr(entries), cap, ptr(scratch), stream_ptr()), "dgnn_point_mesh_distance")
    return d2, dist, face, closest, region, stats


@on_device_of
def point_mesh_distance(vertices, faces, points, grid_resolution=None, return_stats=False, return_d2=False):
    """The distance from each point (fp16 / fp32 / fp64 [n, 3], promoted to fp64) to the mesh (vertices [V, 3], faces int [F, 3]), with where
    it is attained (dgnn_point_mesh_distance; the rule, operation by operation, and the tie rule are in include/dgnn_hip.h).
    -> (dist fp64 [n] = sqrt(d2), correctly rounded, face int32 [n], closest fp64 [n, 3], region uint8 [n]: 0 the face's interior, 1..3 on its edge (v0 v1), (v1 v2),
    (v2 v0), 4..6 at its vertex 0, 1, 2), all on the GPU; with return_d2 the squared distance d2 itself in place of dist; with return_stats also a
    dict of MESH_DISTANCE_STATS -> int.  grid_resolution sizes the candidate grid (None: default_grid_resolution of the face count; 0: no grid,
    every face is tested for every point: the faster call when the queries lie far from the surface, profiles/mesh_distance.md); the answer does
    not depend on it.  ValueError for a mesh without faces, a face id out of range, a
    non-finite referenced vertex or point; DgnnError for a grid_resolution outside [0, 1024]."""
    d2, dist, face, closest, region, stats = _point_mesh_d2(vertices, faces, points, grid_resolution, "point_mesh_distance")
    out = (d2 if return_d2 else dist, face, closest, region)
    return out + (_stats_dict(MESH_DISTANCE_STATS, stats),) if return_stats else out


@on_device_of
def distance_fold(dist, cosine=None, thresholds=()):
    """What the surface metrics need of a list of distances (dgnn_distance_fold): -> (sum of dist, sum of |cosine| (0.0 without), max of dist
    (0.0 for none), [#{dist <= t} for t in thresholds]), the sums in fp64 in a fixed order, so that reruns give the same bits.  dist and cosine
    [n] are cast to fp64."""
    dev = _dev_of(dist, cosine)
    d = _on(dist, dev, torch.float64).reshape(-1)
    c = None if cosine is None else _on(cosine, dev, torch.float64).reshape(-1)
    if c is not None and c.numel() != d.numel():
        raise ValueError("distance_fold: %d cosines for %d distances" % (c.numel(), d.numel()))
    n, nt = d.numel(), len(thresholds)
    thr = torch.tensor([float(t) for t in thresholds], dtype=torch.float64).to(dev) if nt else None
    sums = torch.zeros(3, dtype=torch.float64, device=dev)
    counts = torch.zeros(max(nt, 1), dtype=torch.int64, device=dev)
    scratch = _scratch(dev, lib().dgnn_distance_fold_scratch_bytes(n))
    check(lib().dgnn_distance_fold(ptr(d), ptr(c), n, ptr(thr), nt, ptr(sums), ptr(counts), ptr(scratch), stream_ptr()), "dgnn_distance_fold")
    s = sums.cpu()
    return float(s[0]), float(s[1]), float(s[2]), [int(x) for x in counts.cpu()[:nt]]


@on_device_of
def row_dot3(a, ia, b, ib):
    """a[ia[i]] . b[ib[i]] as (x0 y0 + x1 y1) + x2 y2 in fp64 (dgnn_row_dot3): the cosine between two lists of unit normals picked by index.
    ValueError for an index out of range."""
    dev = _dev_of(a, b, ia, ib)
    x, y = _on(a, dev, torch.float64, 3), _on(b, dev, torch.float64, 3)
    i, j = _on(ia, dev, torch.int32).reshape(-1), _on(ib, dev, torch.int32).reshape(-1)
    if i.numel() != j.numel():
        raise ValueError("row_dot3: %d and %d indices" % (i.numel(), j.numel()))
    out = _empty(dev, torch.float64, i.numel())
    scratch = _scratch(dev, 256)
    _check_value(lib().dgnn_row_dot3(ptr(x), x.size(0), ptr(i), ptr(y), y.size(0), ptr(j), i.numel(), ptr(out), ptr(scratch), stream_ptr()), "dgnn_row_dot3")
    return out


def metric_key(name, threshold):
    """the key of a thresholded surface metric: "fscore@0.01" """
    return "%s@%g" % (name, threshold)


def surface_metric_values(fold_ab, n_a, fold_ba, n_b, thresholds, with_normals=True):
    """The surface metrics from the two folds (distance_fold's results: A -> B over n_a samples of A, B -> A over n_b samples of B): accuracy =
    mean A -> B, completeness = mean B -> A, chamfer_mesh = their mean, hausdorff = the larger maximum, precision@t / recall@t = the share of
    A- / B-samples within t, fscore@t = 2PR / (P + R) (0 when P + R == 0), normal_consistency = the mean of the two mean |cosine|."""
    sa, ca, ma, ka = fold_ab
    sb, cb, mb, kb = fold_ba
    out = {"accuracy": sa / n_a, "completeness": sb / n_b}
    out["chamfer_mesh"] = 0.5 * (out["accuracy"] + out["completeness"])
    out["hausdorff"] = max(ma, mb)
    for t, x, y in zip(thresholds, ka, kb):
        p, r = x / n_a, y / n_b
        out[metric_key("precision", t)], out[metric_key("recall", t)] = p, r
        out[metric_key("fscore", t)] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    if with_normals:
        out["normal_consistency"] = 0.5 * (ca / n_a + cb / n_b)
    return out


def empty_surface_metrics(thresholds, with_normals=True):
    """what the surface metrics are when a side has nothing to measure: inf distances, zero scores"""
    inf = float("inf")
    return surface_metric_values((inf, 0.0, inf, [0] * len(thresholds)), 1, (inf, 0.0, inf, [0] * len(thresholds)), 1, thresholds, with_normals)


def surface_metrics(a_vertices, a_faces, b_vertices, b_faces, n_samples, thresholds, seed=0, return_samples=False):
    """Mesh A against mesh B the way the reconstruction benchmarks score: n_samples points drawn on each by area (sample_interface: fp32, seed
    `seed` for A and seed + 1 for B), each sent to the OTHER MESH by point_mesh_distance (no sampling noise on the far side), the cosine between
    the sample's face normal and its closest face's normal (face_normals, row_dot3; a face without area has the zero normal and adds 0), and
    distance_fold.  -> dict of the keys of surface_metric_values.  A side without faces, or whose faces all have the zero normal (no area to
    sample), gives inf distances and zero scores with a warning; any other failure raises.  With return_samples also the dict of what was measured ("a_points", "a_face", "ab_dist", "ab_face", "ab_cosine" and
    the same for b)."""
    thresholds = [float(t) for t in thresholds]
    dev = _dev_of(a_vertices, a_faces, b_vertices, b_faces)
    va, vb = _on(a_vertices, dev, torch.float64, 3), _on(b_vertices, dev, torch.float64, 3)
    fa, fb = _on(a_faces, dev, torch.int32, 3), _on(b_faces, dev, torch.int32, 3)
    n = int(n_samples)
    if n < 1:
        raise ValueError("surface_metrics: n_samples %d < 1" % n)
    if fa.size(0) == 0 or fb.size(0) == 0:
        print("WARNING: a mesh has no faces; surface distances set to inf and scores to 0")
        out = empty_surface_metrics(thresholds)
        return (out, {}) if return_samples else out
    na, nb = face_normals(va, fa), face_normals(vb, fb)
    if not (bool(na.any()) and bool(nb.any())):          # every normal zero: no face has area, nothing to sample
        print("WARNING: a mesh has no area to sample; surface distances set to inf and scores to 0")
        out = empty_surface_metrics(thresholds)
        return (out, {}) if return_samples else out
    pa, ia = sample_interface(va, fa, None, n, seed=seed)
    pb, ib = sample_interface(vb, fb, None, n, seed=seed + 1)
    dab, fab, _, _ = point_mesh_distance(vb, fb, pa)
    dba, fba, _, _ = point_mesh_distance(va, fa, pb)
    cab, cba = row_dot3(na, ia, nb, fab), row_dot3(nb, ib, na, fba)
    out = surface_metric_values(distance_fold(dab, cab, thresholds), n, distance_fold(dba, cba, thresholds), n, thresholds)
    if return_samples:
        return out, dict(a_points=pa, a_face=ia, ab_dist=dab, ab_face=fab, ab_cosine=cab, b_points=pb, b_face=ib, ba_dist=dba, ba_face=fba, ba_cosine=cba)
    return out


# ---- exact k nearest neighbours and the scan operations on them (csrc/knn.hip) ---------------------------------------------
KNN_STATS = ("shells", "candidates", "placed")
KNN_MAX_K = 64
KNN_CELLS_PER_SQRT_POINT = 0.175


def default_knn_resolution(n_points):
    """The grid resolution ops.knn takes when none is given: 0.175 sqrt(n_points) cells along the longest axis, within [1, 512] -- on a scanned
    surface, whose points fill about 3 R^2 of the R^3 cells, some ten points per occupied cell: the fastest or within 5 % of it at k = 8, 16, 32
    and 64 on scans of 150 000 and 1 000 000 points (the sweep is in profiles/knn.md).  The answer does not depend on it."""
    return max(1, min(512, int(round(KNN_CELLS_PER_SQRT_POINT * float(n_points) ** 0.5))))


@on_device_of
def knn(points, k, queries=None, grid_resolution=None, return_stats=False):
    """The k nearest of `points` (fp16 / fp32 / fp64 [n, 3], promoted to fp64) for every query, exactly (dgnn_knn; the rule and the tie rule
    are in include/dgnn_hip.h): -> (idx int32 [Q, k], d2 fp64 [Q, k]) on the GPU, each row ascending in (d2, index).  queries None: the points
    are their own queries and query i leaves out point i by index (a duplicate of it is its neighbour at d2 = 0); with queries [Q, 3] nothing is
    left out.  Where fewer than k points qualify the row ends in idx = -1, d2 = +inf.  grid_resolution sizes the candidate grid (None:
    default_knn_resolution of the point count; 0: no grid, every point is tested for every query); the answer does not depend on it.  With
    return_stats also a dict of KNN_STATS -> int, summed over the call.  ValueError for k outside [1, 64] and for a non-finite coordinate;
    DgnnError for a grid_resolution outside [0, 1024]."""
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError("knn: k = %d outside [1, %d]" % (k, KNN_MAX_K))
    dev = _dev_of(points, queries)
    p = _points64(points, dev)
    q = None if queries is None else _points64(queries, dev)
    n, nq = p.size(0), (p.size(0) if q is None else q.size(0))
    R = default_knn_resolution(n) if grid_resolution is None else int(grid_resolution)
    scratch = _scratch(dev, lib().dgnn_knn_scratch_bytes(n, R))
    idx, d2 = _empty(dev, torch.int32, nq, k), _empty(dev, torch.float64, nq, k)
    stats = torch.zeros(len(KNN_STATS), dtype=torch.int64, device=dev)
    _check_value(lib().dgnn_knn(ptr(p), n, ptr(q), nq, k, R, ptr(idx), ptr(d2), ptr(stats), ptr(scratch), stream_ptr()), "dgnn_knn")
    return (idx, d2, _stats_dict(KNN_STATS, stats)) if return_stats else (idx, d2)


@on_device_of
def knn_mean_distance(d2, idx):
    """m fp64 [n]: per row of ops.knn's (d2, idx) [n, k] the sum of sqrt(d2) over the valid entries (idx >= 0), in rank order, divided by
    their number (dgnn_knn_mean_distance); a row without a valid entry gives 0 / 0."""
    dev = _dev_of(d2, idx)
    d = _on(d2, dev, torch.float64)
    i = _on(idx, dev, torch.int32)
    if d.dim() != 2 or d.shape != i.shape or d.size(1) < 1:
        raise ValueError("knn_mean_distance: d2 %s and idx %s must be one [n, k] shape" % (tuple(d.shape), tuple(i.shape)))
    n, k = d.shape
    m = _empty(dev, torch.float64, n)
    check(lib().dgnn_knn_mean_distance(ptr(d), ptr(i), n, k, ptr(m), stream_ptr()), "dgnn_knn_mean_distance")
    return m


@on_device_of
def outlier_mask(points, k=16, std_ratio=2.0, grid_resolution=None):
    """Statistical outlier removal (PCL / Open3D, with the population deviation): m_i = the mean distance from point i to its min(k, n - 1)
    nearest neighbours (knn, knn_mean_distance), mu = sum(m) / n, sigma = sqrt(sum((m_i - mu)^2) / n), both sums in a fixed order,
    threshold = mu + std_ratio sigma, keep_i = m_i <= threshold (dgnn_outlier_mask).  -> (keep bool [n] on the GPU, dict of mean_distance
    (fp64 [n], on the GPU), mu, sigma, threshold, n_removed).  ValueError for fewer than 2 points."""
    dev = _dev_of(points)
    p = _points64(points, dev)
    n = p.size(0)
    if n < 2:
        raise ValueError("outlier_mask: %d points, at least 2 are needed" % n)
    idx, d2 = knn(p, min(int(k), n - 1), grid_resolution=grid_resolution)
    m = knn_mean_distance(d2, idx)
    keep = _empty(dev, torch.uint8, n)
    values = torch.zeros(3, dtype=torch.float64, device=dev)
    removed = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = _scratch(dev, lib().dgnn_outlier_mask_scratch_bytes(n))
    _check_value(lib().dgnn_outlier_mask(ptr(m), n, float(std_ratio), ptr(keep), ptr(values), ptr(removed), ptr(scratch), stream_ptr()), "dgnn_outlier_mask")
    v = values.cpu()
    return keep.bool(), {"mean_distance": m, "mu": float(v[0]), "sigma": float(v[1]), "threshold": float(v[2]), "n_removed": int(removed.item())}


@on_device_of
def estimate_normals(points, k=16, sensors=None, grid_resolution=None):
    """PCA normals: for every point the eigenvector of the smallest eigenvalue of the scatter matrix of (the point, then its min(k, n - 1)
    nearest neighbours in rank order), by six cyclic Jacobi sweeps (dgnn_knn_normals; every operation is in include/dgnn_hip.h).  Its sign
    makes the component of largest magnitude positive; with sensors [n, 3] it is negated where n . (sensor - point) < 0, the rule of
    scan_mesh's own normals.  -> (normals fp64 [n, 3], eigenvalues fp64 [n, 3] ascending) on the GPU.  ValueError for fewer than 3 points."""
    dev = _dev_of(points, sensors)
    p = _points64(points, dev)
    n = p.size(0)
    if n < 3:
        raise ValueError("estimate_normals: %d points, at least 3 are needed" % n)
    s = None if sensors is None else _points64(sensors, dev)
    if s is not None and s.size(0) != n:
        raise ValueError("estimate_normals: %d sensors for %d points" % (s.size(0), n))
    idx, d2 = knn(p, min(int(k), n - 1), grid_resolution=grid_resolution)
    normals, eig = _empty(dev, torch.float64, n, 3), _empty(dev, torch.float64, n, 3)
    scratch = _scratch(dev, 256)
    _check_value(lib().dgnn_knn_normals(ptr(p), n, ptr(idx), idx.size(1), ptr(s), ptr(normals), ptr(eig), ptr(scratch), stream_ptr()), "dgnn_knn_normals")
    return normals, eig


# ---- subsampling a scan: voxel grid and exact minimum-distance thinning (csrc/scansub.hip) -----------------------------------
THIN_STATS = ("n_kept", "rounds", "candidates")
THIN_MAX_RESOLUTION = 512
THIN_CELLS_PER_RADIUS = 0.25


@on_device_of
def voxel_subsample(points, voxel_size, origin=(0.0, 0.0, 0.0)):
    """One row per occupied voxel of edge `voxel_size` (dgnn_voxel_subsample; the rule is in include/dgnn_hip.h): a point's voxel is
    floor((x - origin) / voxel_size) per axis, the voxels are numbered by their lowest member.  -> dict on the GPU: "voxel" int32 [n] (the
    point's voxel row), "count" int32 [m], "first" int32 [m] (the lowest member), "centroid" fp64 [m, 3] (the members summed in ascending
    index, fixed_sum.h's order), "nearest" int32 [m] (the member with the smallest (d2 to the centroid, index)), and "m".  The same input
    gives the same bytes.  ValueError for a voxel_size that is not finite and positive, a non-finite coordinate, and a voxel coordinate
    outside (-2^20, 2^20)."""
    dev = _dev_of(points)
    p = _points64(points, dev)
    n = p.size(0)
    org = (C.c_double * 3)(*[float(x) for x in origin])
    voxel, count, first, nearest = (_empty(dev, torch.int32, n) for _ in range(4))
    centroid = _empty(dev, torch.float64, n, 3)
    m = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = _scratch(dev, lib().dgnn_voxel_subsample_scratch_bytes(n))
    _check_value(lib().dgnn_voxel_subsample(ptr(p), n, float(voxel_size), org, ptr(voxel), ptr(count), ptr(first), ptr(centroid), ptr(nearest), ptr(m),
                                            ptr(scratch), stream_ptr()), "dgnn_voxel_subsample")
    m = int(m.item())
    return dict(voxel=voxel, count=count[:m], first=first[:m], centroid=centroid[:m], nearest=nearest[:m], m=m)


def default_thin_resolution(extent, radius):
    """The grid resolution ops.min_distance_thin takes when none is given: floor(0.25 extent / radius) cells along the longest axis (extent:
    its length), within [1, 512]: a cell's edge is four radii, and a point reads 8 to 27 cells.  A choice, not a need: the answer is the same
    at every resolution.  One cell per radius, the natural first guess, reads a quarter of the candidates but was 6 - 25 % slower on scans of
    150 000 and 999 997 points at 1, 2 and 4 mean spacings: its cells hold a point or two, so a wavefront reads 27 nearly empty runs (the
    sweep is in profiles/scan_subsample.md)."""
    extent, radius = float(extent), float(radius)
    if not (extent > 0.0 and radius > 0.0):          # no extent, radius 0 (nothing conflicts), or a NaN (the library refuses it): one cell
        return 1
    cells = THIN_CELLS_PER_RADIUS * extent / radius
    return THIN_MAX_RESOLUTION if cells >= THIN_MAX_RESOLUTION else max(1, int(cells))


@on_device_of
def min_distance_thin(points, radius, priority=None, seed=0, grid_resolution=None, return_stats=False):
    """Exact minimum-distance (Poisson-disk) thinning (dgnn_min_distance_thin; the rule is in include/dgnn_hip.h): points i and j conflict iff
    d2(i, j) < radius^2; the points are walked in the order of (key_i, i) -- key_i = priority[i] (int64, lower first), or without one the
    splitmix64 hash of (seed, i) -- and a point is kept iff it conflicts with no point kept before it.  -> keep bool [n] on the GPU, the
    lexicographically first maximal independent set; with return_stats also a dict of THIN_STATS -> int.  grid_resolution sizes the candidate
    grid (None: default_thin_resolution of the longest extent; 0: all pairs); the answer does not depend on it.  ValueError for a radius that
    is not finite and >= 0 and for a non-finite coordinate; DgnnError for a grid_resolution outside [0, 1024]."""
    dev = _dev_of(points, priority)
    p = _points64(points, dev)
    n = p.size(0)
    pr = None
    if priority is not None:
        pr = _on(priority, dev, torch.int64).reshape(-1)
        if pr.numel() != n:
            raise ValueError("min_distance_thin: %d priorities for %d points" % (pr.numel(), n))
    if grid_resolution is None:
        R = default_thin_resolution(float((p.max(dim=0).values - p.min(dim=0).values).max()), radius) if n else 1
    else:
        R = int(grid_resolution)
    scratch = _scratch(dev, lib().dgnn_min_distance_thin_scratch_bytes(n, R))
    keep = _empty(dev, torch.uint8, n)
    stats = torch.zeros(len(THIN_STATS), dtype=torch.int64, device=dev)
    _check_value(lib().dgnn_min_distance_thin(ptr(p), n, float(radius), ptr(pr), int(seed) & 0xFFFFFFFFFFFFFFFF, R, ptr(keep), ptr(stats), ptr(scratch),
                                              stream_ptr()), "dgnn_min_distance_thin")
    return (keep.bool(), _stats_dict(THIN_STATS, stats)) if return_stats else keep.bool()


# ---- ingest: feature scaling (csrc/ingest.hip) ------------------------------------------------------------------------------------
SCALE_KINDS = {"none": 0, "standard": 1, "minmax": 2, "robust": 3}


def _col_range(r, c, name):
    if r is None:
        return 0, 0
    a, b = int(r[0]), int(r[1])
    if not 0 <= a <= b <= c:
        raise ValueError("%s=%r outside the frame's columns [0, %d]" % (name, r, c))
    return a, b


@on_device_of
def scale_features(x64, c_first: int, kind: str, feature_range=(0, 1), sum_cols=None, div_col=None, div_cols=None, div_scalar=None, scalar_cols=None,
                   return_stats=False):
    """fp64 [n, c] frame (rows may be strided) -> fp32 [n, c]: the reference's feature scaling (processing/data.py:444-506 + the float32 cast).
    Pre-steps, in this order, in fp64, each over a column range (c0, c1) or None: `sum_cols` x*1000/colsum; `div_cols` x/(x[:, div_col] + 1e-4)
    with the divisor taken after the sum step; `scalar_cols` x/div_scalar.  Then the scaler `kind` -- "none", "standard", "minmax" (onto
    `feature_range`) or "robust" -- fitted on the pre-transformed columns >= c_first; columns below are only pre-transformed and cast.
    return_stats: -> (out, stats fp64 [2, c]): what was subtracted and what was divided by (minmax: data_min and the zero-handled range)."""
    _req(x64, "x64", torch.float64, dim=2)
    if kind not in SCALE_KINDS:
        raise ValueError("kind=%r: one of %s" % (kind, sorted(SCALE_KINDS)))
    n, c = x64.shape
    if n < 1 or c < 1 or not 0 <= int(c_first) <= c:
        raise ValueError("scale_features: frame %s, c_first %r" % (tuple(x64.shape), c_first))
    s0, s1 = _col_range(sum_cols, c, "sum_cols")
    d0, d1 = _col_range(div_cols, c, "div_cols")
    k0, k1 = _col_range(scalar_cols, c, "scalar_cols")
    if d0 < d1 and (div_col is None or not 0 <= int(div_col) < c):
        raise ValueError("div_cols needs div_col in [0, %d), got %r" % (c, div_col))
    if k0 < k1 and div_scalar is None:
        raise ValueError("scalar_cols needs div_scalar")
    dev = x64.device
    out = torch.empty((n, c), dtype=torch.float32, device=dev)
    stats = torch.empty((2, c), dtype=torch.float64, device=dev) if return_stats else None
    scratch = _scratch(dev, lib().dgnn_scale_features_scratch_bytes(c))
    check(lib().dgnn_scale_features_f64(ptr(x64), _ld(x64), n, c, int(c_first), SCALE_KINDS[kind], float(feature_range[0]), float(feature_range[1]),
                                        s0, s1, int(div_col or 0), d0, d1, float(div_scalar if div_scalar is not None else 1.0), k0, k1,
                                        ptr(out), c, ptr(stats), ptr(scratch), stream_ptr()), "dgnn_scale_features_f64")
    return (out, stats) if return_stats else out


# ---- exact in-sphere predicate, 3D Delaunay triangulation, its certificate (csrc/exact_insphere.h, csrc/delaunay.hip) ----
DELAUNAY_STATS = ("rounds", "points_per_round_min", "points_per_round_max", "max_cavity", "exact_insphere", "exact_orient", "cells_allocated",
                  "need", "dup_a", "dup_b", "slow_paths")
VIOLATIONS = ("flat", "negative", "nonlocal_facets", "concave_hull_edges", "bad_links")
_E_CAPACITY, _E_DUPLICATE = -5, -6
_EVEN_PERMS = ((0, 1, 2, 3), (0, 2, 3, 1), (0, 3, 1, 2), (1, 0, 3, 2), (1, 2, 0, 3), (1, 3, 2, 0), (2, 0, 1, 3), (2, 1, 3, 0), (2, 3, 0, 1),
               (3, 0, 2, 1), (3, 1, 0, 2), (3, 2, 1, 0))
# the facet opposite slot s of a positive tet, ordered so that the tet's own vertex s -- and so every point -- lies on its negative side
_OUTWARD_FACET = ((1, 2, 3), (0, 3, 2), (0, 1, 3), (0, 2, 1))


@on_device_of
def insphere_sign(points5):
    """(signs int8 [n] on the GPU, exact-stage calls int) of dgnn_insphere_sign for points5 fp64 [n, 5, 3] = (a, b, c, d, e) per case: +1 when e
    lies strictly inside the sphere through a..d, 0 on it, -1 outside; 0 for flat a..d.  Exact for coordinates that are 0 or of a magnitude
    in [2^-150, 2^150]; DgnnError outside that range (NaN and infinities included)."""
    dev = _dev_of(points5)
    p = torch.as_tensor(points5).to(dev, torch.float64).contiguous()
    if p.dim() != 3 or tuple(p.shape[1:]) != (5, 3):
        raise ValueError("expected [n, 5, 3], got %s" % (tuple(p.shape),))
    n = p.size(0)
    out = _empty(dev, torch.int8, n)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    check(lib().dgnn_insphere_sign(ptr(p), n, ptr(out), ptr(counts), stream_ptr()), "dgnn_insphere_sign")
    return out, int(counts[0].item())


def delaunay_priority(n, seed=0, device=None):
    """The default insertion order of `delaunay`: the rank of point i is its place in the ascending order of mm_hash(seed, i) (the counter hash
    of include/dgnn_hip.h, 64 bits, unsigned; ties by index) -> (order int64 [n]: order[r] = the point of rank r) on `device`."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    m34, m37, m33 = (1 << 34) - 1, (1 << 37) - 1, (1 << 33) - 1

    def s64(x):   # a 64-bit constant as the int64 with the same bits
        x &= (1 << 64) - 1
        return x - (1 << 64) if x >> 63 else x

    z = torch.arange(n, dtype=torch.int64, device=dev) * s64(0x9E3779B97F4A7C15) + s64(int(seed))   # int64 arithmetic wraps: the uint64 bits
    z = (z ^ ((z >> 30) & m34)) * s64(0xBF58476D1CE4E5B9)
    z = (z ^ ((z >> 27) & m37)) * s64(0x94D049BB133111EB)
    z = z ^ ((z >> 31) & m33)
    return torch.sort(z ^ s64(1 << 63), stable=True)[1]   # the sign bit flipped: signed order = unsigned order


@on_device_of
def delaunay(points, priority=None, seed=0, cell_capacity=None):
    """The Delaunay triangulation of distinct fp64 points [n, 3] (dgnn_delaunay; contract in include/dgnn_hip.h) -> dict on the GPU:
      "tetrahedra" int32 [T, 4]: the finite cells, each with its smallest vertex id first and, among the row's even permutations, the
          lexicographically smallest; det[v1 - v0, v2 - v0, v3 - v0] > 0 exactly; rows sorted lexicographically;
      "neighbors" int32 [T + H, 4]: cells T..T+H-1 are the infinite cells, one per hull facet, ordered by (finite cell, slot).  Slot k of a
          finite cell: the cell across the facet opposite vertex k.  Slot 0 of an infinite cell: its finite cell; slots 1..3: the infinite
          cells across the hull edges opposite the three vertices of its row in "hull_facets";
      "hull_facets" int32 [H, 3]: every input point lies on or behind each (orient <= 0);
      "stats": rounds, points_per_round_min / _max, max_cavity, exact_insphere, exact_orient (exact-stage calls), capacity_retries,
          slow_paths, cells_allocated, cell_capacity, workspace_bytes.
    priority: an int permutation [n], the point of the lowest value goes first where points contend; None: the order of delaunay_priority(n,
    seed).  In general position the result does not depend on either.  cell_capacity: cells of storage (default about 8 n + 64; doubled
    and retried when too small).  ValueError: n < 4, non-finite coordinates, a priority that is no permutation.  DgnnError: coordinates outside
    the predicate's range, a duplicate point (the pair is named), all points coplanar."""
    dev = _dev_of(points)
    p = _on(points, dev, torch.float64, 3)
    n = p.size(0)
    if n < 4:
        raise ValueError("delaunay: %d points, at least 4 are needed" % n)
    if not bool(torch.isfinite(p).all()):
        raise ValueError("delaunay: a coordinate is not finite")
    if priority is None:
        order = delaunay_priority(n, seed, dev)
    else:
        pr = torch.as_tensor(priority)
        if pr.dtype.is_floating_point or pr.dtype == torch.bool or pr.dim() != 1 or pr.numel() != n:
            raise ValueError("delaunay: priority must be an int permutation [%d]" % n)
        pr = pr.to(dev, torch.int64)
        srt, order = torch.sort(pr, stable=True)
        if not bool((srt == torch.arange(n, device=dev)).all()):
            raise ValueError("delaunay: priority is not a permutation of 0..%d (ties are refused)" % (n - 1))
    pts = p[order].contiguous()
    cap = int(cell_capacity) if cell_capacity is not None else int(lib().dgnn_delaunay_default_capacity(n))
    cap, retries = max(cap, 5), 0
    while True:
        cells, nbrs = _empty(dev, torch.int32, cap, 4), _empty(dev, torch.int32, cap, 4)
        nbytes = int(lib().dgnn_delaunay_scratch_bytes(n, cap))
        scratch = _scratch(dev, nbytes, "delaunay: %d points with %d cells exceed the int32 indexing" % (n, cap))
        st = (C.c_int64 * 16)()
        code = lib().dgnn_delaunay(ptr(pts), n, cap, ptr(cells), ptr(nbrs), st, ptr(scratch), stream_ptr())
        if code == _E_CAPACITY:
            cap, retries = max(2 * cap, int(st[DELAUNAY_STATS.index("need")])), retries + 1
            continue
        if code == _E_DUPLICATE:
            a, b = int(order[int(st[DELAUNAY_STATS.index("dup_a")])]), int(order[int(st[DELAUNAY_STATS.index("dup_b")])])
            raise DgnnError("delaunay: points %d and %d are equal" % (min(a, b), max(a, b)))
        _check_value(code, "dgnn_delaunay")
        break
    raw = _stats_dict(DELAUNAY_STATS, st)
    nc = raw["cells_allocated"]
    tv, tn = cells[:nc].long(), nbrs[:nc].long()
    alive = tv[:, 0] >= 0
    ghost = alive & (tv == n).any(dim=1)
    fin_ids = torch.nonzero(alive & ~ghost).reshape(-1)
    vmap = torch.cat([order, torch.full((1,), -1, dtype=torch.int64, device=dev)])
    v = vmap[tv[fin_ids]]                                                  # original ids of the finite cells' vertices
    perms = torch.tensor(_EVEN_PERMS, dtype=torch.int64, device=dev)
    k1 = v[:, perms[:, 0]] * (n + 1) + v[:, perms[:, 1]]                   # the first two vertices fix an even permutation
    sel = perms[torch.argmin(k1, dim=1)]
    tets, nb_raw = torch.gather(v, 1, sel), torch.gather(tn[fin_ids], 1, sel)
    srt = torch.sort(tets[:, 2] * (n + 1) + tets[:, 3], stable=True)[1]
    srt = srt[torch.sort((tets[:, 0] * (n + 1) + tets[:, 1])[srt], stable=True)[1]]
    tets, nb_raw, fin_ids = tets[srt], nb_raw[srt], fin_ids[srt]
    T = tets.size(0)
    hpos = torch.nonzero(ghost[nb_raw].reshape(-1)).reshape(-1)           # (finite cell, slot) of the hull facets, ascending
    H = hpos.numel()
    inf_raw = nb_raw.reshape(-1)[hpos]
    newidx = torch.full((nc,), -1, dtype=torch.int64, device=dev)
    newidx[fin_ids] = torch.arange(T, device=dev)
    newidx[inf_raw] = T + torch.arange(H, device=dev)
    hi, hs = hpos // 4, hpos % 4
    facet_slots = torch.tensor(_OUTWARD_FACET, dtype=torch.int64, device=dev)[hs]
    hull = torch.gather(tets[hi], 1, facet_slots)
    ov = vmap[tv[inf_raw]]                                                 # the infinite cells' vertices, -1 = the ghost
    inf_nb = torch.empty((H, 4), dtype=torch.int64, device=dev)
    inf_nb[:, 0] = hi
    for j in range(3):
        pos = (ov == hull[:, j:j + 1]).int().argmax(dim=1, keepdim=True)
        inf_nb[:, j + 1] = newidx[torch.gather(tn[inf_raw], 1, pos).reshape(-1)]
    neighbors = torch.cat([newidx[nb_raw], inf_nb]).to(torch.int32)
    if T == 0 or int(neighbors.min()) < 0:
        raise DgnnError("delaunay: the cells do not close up (%d finite, %d infinite)" % (T, H))
    stats = {k: raw[k] for k in ("rounds", "points_per_round_min", "points_per_round_max", "max_cavity", "exact_insphere", "exact_orient",
                                 "slow_paths", "cells_allocated")}
    stats.update(capacity_retries=retries, cell_capacity=cap, workspace_bytes=nbytes + 2 * cells.numel() * 4)
    return {"tetrahedra": tets.to(torch.int32), "neighbors": neighbors, "hull_facets": hull.to(torch.int32), "stats": stats}


def facet_neighbors(tetrahedra):
    """(neighbors int64 [T, 4] with -1 where no cell lies across, facets shared by more than two cells) of any cell list, by matching the
    sorted vertex triples of the facets (torch sort on the GPU).  Slot k is the facet opposite vertex k."""
    t = tetrahedra.long()
    T = t.size(0)
    dev = t.device
    opp = torch.tensor(((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2)), dtype=torch.int64, device=dev)
    f = torch.sort(t[:, opp], dim=2)[0].reshape(-1, 3)
    _, inv, counts = torch.unique(f, dim=0, return_inverse=True, return_counts=True)
    nbr = torch.full((4 * T,), -1, dtype=torch.int64, device=dev)
    order = torch.sort(inv, stable=True)[1]
    si = inv[order]
    pair = (si[1:] == si[:-1]) & (counts[si[1:]] == 2)
    a, b = order[:-1][pair], order[1:][pair]
    nbr[a], nbr[b] = b // 4, a // 4
    return nbr.reshape(T, 4), int((counts > 2).sum())


@on_device_of
def delaunay_violations(vertices, tetrahedra):
    """A certificate for any `_3dt`-style cell list (dgnn_delaunay_violations on the neighbours of facet_neighbors), all exact -> dict of
    counts: "flat" and "negative" cells, "overfull_facets" (more than two cells), "nonlocal_facets" (interior facets whose opposite vertex
    lies strictly inside the cell's sphere), "concave_hull_edges" ((hull facet, edge) pairs where the next hull facet's apex lies strictly
    beyond the facet), "bad_links".  All zero for a Delaunay triangulation of its vertices' hull."""
    dev = _dev_of(vertices, tetrahedra)
    v = _on(vertices, dev, torch.float64, 3)
    tets = _on(tetrahedra, dev, torch.int32, 4)
    T = tets.size(0)
    if T and (int(tets.min()) < 0 or int(tets.max()) >= v.size(0)):
        raise DgnnError("delaunay_violations: a vertex id out of range")
    nbr, overfull = facet_neighbors(tets) if T else (torch.zeros((0, 4), dtype=torch.int64, device=dev), 0)
    nbr = nbr.to(torch.int32).contiguous()
    counts = torch.zeros(len(VIOLATIONS) + 1, dtype=torch.int64, device=dev)
    check(lib().dgnn_delaunay_violations(ptr(v), v.size(0), ptr(tets), ptr(nbr), T, ptr(counts), stream_ptr()), "dgnn_delaunay_violations")
    out = _stats_dict(VIOLATIONS, counts[:len(VIOLATIONS)])
    out["overfull_facets"] = overfull
    return out


# ---- singular vertices and their repair by relabelling cells (csrc/manifold.hip) ------------------------------------------
MANIFOLD_STATS = ("rounds", "moves", "flipped_cells", "to_inside", "to_outside", "flipped_cost", "singular_before", "singular_after")


def _labelled_cells(tetrahedra, neighbors, labels, what):
    dev = _dev_of(labels, tetrahedra, neighbors)
    tets = _on(tetrahedra, dev, torch.int32, 4)
    nbr = _on(neighbors, dev, torch.int32, 4)
    lab = _on(labels, dev, torch.int32).reshape(-1)
    if nbr.size(0) != tets.size(0) or lab.numel() != tets.size(0):
        raise ValueError("%s: %d cells, %d neighbour rows, %d labels" % (what, tets.size(0), nbr.size(0), lab.numel()))
    return dev, tets, nbr, lab


@on_device_of
def vertex_components(tetrahedra, neighbors, labels, n_vertices):
    """(n_inside int32 [V], n_outside int32 [V], n_singular) of dgnn_vertex_components: per vertex the connected components a(v) of the
    inside cells (label 0) and b(v) of the outside cells (label 1, the infinite cell among them) of its star, two cells joined when they
    share a facet through the vertex and carry the same label; a vertex is singular when a > 1 or b > 1, and the interface of the labels is
    a closed manifold surface exactly when none is.  tetrahedra int [T, 4], neighbors int [T, 4] slot-wise with -1 = the
    infinite cell (tet_neighbors; of `delaunay`: the first T rows with ids >= T set to -1).  DgnnError for malformed input."""
    dev, tets, nbr, lab = _labelled_cells(tetrahedra, neighbors, labels, "vertex_components")
    t, nv = tets.size(0), int(n_vertices)
    n_in, n_out = _zeros(dev, torch.int32, nv), _zeros(dev, torch.int32, nv)
    scratch = _scratch(dev, lib().dgnn_vertex_components_scratch_bytes(t, nv), "vertex_components: %d cells with %d vertices exceed the int32 indexing" % (t, nv))
    n_singular = C.c_int64(0)
    check(lib().dgnn_vertex_components(ptr(tets), ptr(nbr), ptr(lab), t, nv, ptr(n_in), ptr(n_out), C.byref(n_singular), ptr(scratch), stream_ptr()),
          "dgnn_vertex_components")
    return n_in, n_out, int(n_singular.value)


@on_device_of
def manifold_repair(tetrahedra, neighbors, labels, n_vertices, cost=None, max_rounds=None, return_flipped=False):
    """Relabels cells until no vertex is singular or no move is left (dgnn_manifold_repair; the rule is in include/dgnn_hip.h):
    per round every singular vertex offers its cheapest component -- by (sum of `cost`, smallest cell id) -- that holds neither the infinite
    cell nor an already flipped cell, the vertices that own their whole star win, and the winners' components change side.  A cell flips at
    most once.  cost: int [T], each >= 0 (None: all ones, the fewest cells flip).  max_rounds only stops early: the result after r rounds.
    -> (labels int32 [T] on the GPU (a new tensor), stats dict of MANIFOLD_STATS; singular_after = the stuck vertices of a call that ran to
    its end) (+ flipped int32 [T] with return_flipped).  DgnnError for malformed input."""
    dev, tets, nbr, lab = _labelled_cells(tetrahedra, neighbors, labels, "manifold_repair")
    t, nv = tets.size(0), int(n_vertices)
    out = lab.clone()
    cst = None
    if cost is not None:
        cst = _on(cost, dev, torch.int32).reshape(-1)
        if cst.numel() != t:
            raise ValueError("manifold_repair: %d costs for %d cells" % (cst.numel(), t))
    flipped = _zeros(dev, torch.int32, t) if return_flipped else None
    scratch = _scratch(dev, lib().dgnn_manifold_repair_scratch_bytes(t, nv), "manifold_repair: %d cells with %d vertices exceed the int32 indexing" % (t, nv))
    st = (C.c_int64 * len(MANIFOLD_STATS))()
    check(lib().dgnn_manifold_repair(ptr(tets), ptr(nbr), ptr(out), ptr(cst), t, nv, -1 if max_rounds is None else max(int(max_rounds), 0),
                                     ptr(flipped), st, ptr(scratch), stream_ptr()), "dgnn_manifold_repair")
    stats = _stats_dict(MANIFOLD_STATS, st)
    return (out, stats, flipped) if return_flipped else (out, stats)
