"""fp64 restatements (plain torch / numpy) of the fp32 streaming kernels around the fused layers, written from the formulas in the headers of
csrc/norm.hip and csrc/adam.hip: BatchNorm1d's batch statistics with the running buffers, the scale / shift fold, the backward of
y = relu(bn(x)) in its one-piece and its two-rank (`count`) form, and one Adam step -- in fp64, and op for op in numpy.float32 in the kernel's
order.  The BatchNorm functions follow the device of their arguments (a test may keep the fp64 side of a 70 001 x 1024 case on the GPU); nothing
here calls the library."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch


# ---- BatchNorm1d ---------------------------------------------------------------------------------
def bn_stats(X, rm0=None, rv0=None, momentum=0.1):
    """-> (mean, biased var, running mean, running var) of the rows of X [M, c]; the running buffers take momentum * (mean, UNBIASED var), and a
    single row, which has no unbiased variance, keeps the biased value (0)"""
    M = X.shape[0]
    mean = X.mean(0)
    var = (X - mean).pow(2).mean(0)
    unb = var * (M / (M - 1)) if M > 1 else var
    rm = None if rm0 is None else (1 - momentum) * rm0 + momentum * mean
    rv = None if rv0 is None else (1 - momentum) * rv0 + momentum * unb
    return mean, var, rm, rv


def bn_fold(gamma, beta, mean, var, eps):
    """y = x * scale + shift: scale = gamma / sqrt(var + eps), shift = beta - mean * scale (no gamma: 1, no beta: 0)"""
    scale = 1.0 / torch.sqrt(var + eps)
    if gamma is not None:
        scale = gamma * scale
    shift = -mean * scale
    if beta is not None:
        shift = beta + shift
    return scale, shift


BnBwd = namedtuple("BnBwd", "dx dgamma dbeta mag_dx mag_dgamma mag_dbeta")


def bn_relu_bwd(X, Y, DY, gamma, mean, var, eps, train, relu, count=None, sums=None):
    """Backward of y = relu(bn(x)) for the rows X: g = dy behind the mask [y > 0] (relu) or dy itself,
         dbeta = sum g,  dgamma = sum g * xhat,  xhat = (x - mean) / sqrt(var + eps),
         train: dx = gamma / sqrt(var + eps) * (g - dbeta / n - xhat * dgamma / n)        eval: dx = g * gamma / sqrt(var + eps).
    `count` (two-rank form): n, the number of rows the statistics were taken over, when these rows are only a part of them; `sums` =
    (dbeta, dgamma) over all `count` rows then (default: the sums of these rows).  dbeta / dgamma returned are always the sums over THESE rows.
    The magnitude terms are what a rounding bound multiplies: per column sum |g| and sum |g| |xhat|, per element the terms of dx with every
    sign made positive."""
    M = X.shape[0]
    g = DY * (Y > 0) if relu else DY
    inv = 1.0 / torch.sqrt(var + eps)
    xh = (X - mean) * inv
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    mag_dbeta, mag_dgamma = g.abs().sum(0), (g.abs() * xh.abs()).sum(0)
    gs = inv if gamma is None else gamma * inv
    if train:
        n = float(M if count is None else count)
        sb, sg = (dbeta, dgamma) if sums is None else sums
        dx = gs * (g - sb / n - xh * sg / n)
        mb, mg = (mag_dbeta, mag_dgamma) if sums is None else (sb.abs(), sg.abs())
        mag_dx = gs.abs() * (g.abs() + mb / n + xh.abs() * mg / n)
    else:
        dx = g * gs
        mag_dx = g.abs() * gs.abs()
    return BnBwd(dx, dgamma, dbeta, mag_dx, mag_dgamma, mag_dbeta)


# ---- Adam ----------------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, b1, b2, eps, t):
    """One step of torch.optim.Adam's rule (no amsgrad / weight decay / maximize) on float64 numpy arrays -> (p, m, v):
         m = m + (g - m) (1 - b1)      v = b2 v + (1 - b2) g g      p = p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - math.pow(b1, t), 1.0 - math.pow(b2, t)
    p = p - (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v


def adam_host_scalars(lr, b1, b2, t):
    """the two scalars the host forms in double from the fp32 hyper-parameters and rounds once: (lr / (1 - b1^t), 1 / sqrt(1 - b2^t))"""
    lr, b1, b2 = (float(np.float32(a)) for a in (lr, b1, b2))
    bc1, bc2 = 1.0 - math.pow(b1, t), 1.0 - math.pow(b2, t)
    return np.float32(lr / bc1), np.float32(1.0 / math.sqrt(bc2))


def adam_step_f32(p, g, m, v, lr, b1, b2, eps, t):
    """The same rule op for op in numpy.float32, in the order of the kernel: every line below is one rounded fp32 operation per operator"""
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    lr_over_bc1, inv_bc2_sqrt = adam_host_scalars(lr, b1, b2, t)
    b1, b2, eps = f(b1), f(b2), f(eps)
    w1, w2 = f(1) - b1, f(1) - b2
    with np.errstate(under="ignore"):
        mi = m + (g - m) * w1
        vi = b2 * v + w2 * g * g
        denom = np.sqrt(vi) * inv_bc2_sqrt + eps
        pi = p - lr_over_bc1 * (mi / denom)
    assert mi.dtype == f and vi.dtype == f and pi.dtype == f
    return pi, mi, vi
