"""What the per-kernel suites of the fused SAGE inference layers share (tests/test_gpu_ws.py, tests/test_gpu_fused_edges.py, tests/test_gpu_bf16.py;
tests/test_fused_layer_model_cpu.py holds this file to its own promises): the layer

    y_i = act( ( Wj . mean_{e->i}( x[src_e] * (We . A_e + be) ) + bj + Wi . x_i ) * scale + shift )

in fp64 together with the magnitude of the terms that were added up (the same expression over absolute values: what a bound per element is
proportional to), the decoder behind it, graphs and inputs that reach what the kernels can get wrong, the tile geometry of the two-phase kernels
restated from their sources, and the per-element check with its report.  Pure CPU: nothing here imports the GPU package."""
import numpy as np
import torch

FE = 20                      # edge attributes (fused::FE)
NUM_CU = 256                 # DGNN_NUM_CU (csrc/common.h)
K_F16 = 2.0 ** -19           # f16x2 / f16x2d: 22 significand bits per operand, fp32 accumulation (the bound of tests/test_gpu_ws.py)
K_F32 = 2.0 ** -20           # f32 / bf16x3 / bf16x3f: fp32-class
K_LOGIT = 2.0 ** -18         # decoder logits, on decoder_reference's magnitude
MODES = ("f32", "bf16x3", "bf16x3f", "f16x2d", "f16x2")
KAPPA = {"f32": K_F32, "bf16x3": K_F32, "bf16x3f": K_F32, "f16x2d": K_F16, "f16x2": K_F16}


def _d(t):
    return None if t is None else t.double()


def reference(x, ea, ei, n_dst, We, be, Wj, bj, Wi, scale, shift, relu=True, x_dst=None):
    """fp64: (result, magnitude of the terms that were added up).  `bj`, `scale` / `shift` may be None, `x` may hold more rows than n_dst (source rows
    that are no destinations); the destinations' own rows are x[:n_dst] unless `x_dst` gives them."""
    from oracle.pyg_semantics import propagate_mean
    xd, own = _d(x), _d(x[:n_dst] if x_dst is None else x_dst)
    a = propagate_mean(xd, n_dst, ei, _d(ea) @ _d(We).t() + _d(be))
    amag = propagate_mean(xd.abs(), n_dst, ei, _d(ea).abs() @ _d(We).abs().t() + _d(be).abs())
    ref = a @ _d(Wj).t() + own @ _d(Wi).t()
    mag = amag @ _d(Wj).abs().t() + own.abs() @ _d(Wi).abs().t()
    if bj is not None:
        ref, mag = ref + _d(bj), mag + _d(bj).abs()
    if scale is not None:
        ref, mag = ref * _d(scale) + _d(shift), mag * _d(scale).abs() + _d(shift).abs()
    return (torch.relu(ref) if relu else ref), mag


def decoder_reference(ref, mag, W0, b0, s1, h1, W3, b3):
    """Linear - BatchNorm(eval, folded into s1 / h1) - ReLU - Linear behind the layer's rows, fp64: (logits, magnitude)"""
    hid = torch.relu((ref @ _d(W0).t() + _d(b0)) * _d(s1) + _d(h1))
    lref = hid @ _d(W3).t() + _d(b3)
    lmag = (((mag @ _d(W0).abs().t() + _d(b0).abs()) * _d(s1).abs() + _d(h1).abs()) @ _d(W3).abs().t()) + _d(b3).abs()
    return lref, lmag


# ---- graphs ------------------------------------------------------------------------------------------------------------------------------
STRETCH = 64                          # destinations per stretch: the largest tile of any instantiation, four gather groups of the widest kind (16)
OFF_40, OFF_0, OFF_3, OFF_5 = 0, 2, 47, 63      # where a ragged stretch keeps its in-degree 40 / 0 / 3 / 5 cells


def stretch_is_ragged(s):
    """Stretches alternate between the two kinds in the Thue-Morse order (ragged where the stretch number has an even count of one bits: 0, 3, 5, 6, 9 ...).
    A workgroup walks tiles a power of two apart (32 or 64 at the deep sizes, with 32- and 64-cell tiles): under the plain even / odd order all of its
    tiles would be of one kind and no wave would ever hand over from one path to the other there."""
    s = np.asarray(s, dtype=np.int64)
    p = np.zeros_like(s)
    while (s > 0).any():
        p ^= s & 1
        s = s >> 1
    return p == 0


def ragged_degrees(n_dst, seed):
    """in-degrees of ragged_graph.  A regular stretch: 4 everywhere, so every gather group in it (4, 8 or 16 cells) takes the matrix-core path.  A ragged
    stretch: cells 0 .. 31 drawn from 0 .. 9 with a 40 at cell 0 and a 0 at cell 2; cells 32 .. 47 and 48 .. 63 are groups of 16 with in-degree 4 except for
    their last cell (3 and 5): to a kernel that gathers 4 or 8 cells per wave they are regular groups followed by one the per-lane path takes, to one
    that gathers 16 two more groups of that path."""
    rng = np.random.default_rng(seed)
    i = np.arange(n_dst)
    off = i % STRETCH
    deg = np.where(off < 32, rng.integers(0, 10, n_dst), 4)
    deg[off == OFF_40], deg[off == OFF_0], deg[off == OFF_3], deg[off == OFF_5] = 40, 0, 3, 5
    deg[~stretch_is_ragged(i // STRETCH)] = 4
    return deg.astype(np.int64)


def ragged_graph(n_dst, n_src, seed):
    """edge_index int64 [2, E] with in-degrees ragged_degrees(n_dst, seed), sources from [0, n_src) (call it with n_src = n_dst + 37: rows that are no
    destinations), self-loops (every 7th cell with an edge), duplicate edges (every 5th cell with two) and shuffled columns: the plan's eid is no identity."""
    rng = np.random.default_rng(seed + 1)
    deg = ragged_degrees(n_dst, seed)
    dst = np.repeat(np.arange(n_dst), deg)
    src = rng.integers(0, n_src, dst.shape[0])
    first = np.cumsum(deg) - deg
    loops = np.arange(0, n_dst, 7)
    loops = loops[deg[loops] >= 1]
    src[first[loops]] = loops
    dup = np.arange(3, n_dst, 5)
    dup = dup[deg[dup] >= 2]
    src[first[dup] + 1] = src[first[dup]]
    perm = rng.permutation(dst.shape[0])
    return np.stack([src[perm], dst[perm]]).astype(np.int64)


def regular_graph(n_dst, n_src, seed):
    """four rows per destination in the reference layout (sorted by destination: the plan's eid is the identity)"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, n_src, 4 * n_dst), np.repeat(np.arange(n_dst), 4)]).astype(np.int64)


def in_degrees(ei, n_dst):
    return np.bincount(np.asarray(ei[1]), minlength=n_dst).astype(np.int64)


def group_regular(deg, tpw):
    """per cell: does its gather group of `tpw` cells take the matrix-core path, as fused_mfma.hip decides it (every cell OF THE GRAPH in the group has
    in-degree 4; a short last group counts with the cells it has).  fused.hip sends a short last group down the per-lane path, with the same bits."""
    deg = np.asarray(deg)
    n = deg.shape[0]
    g = np.arange(n) // tpw
    bad = np.bincount(g, weights=(deg != 4), minlength=g.max() + 1 if n else 0)
    return bad[g] == 0


def layer_inputs(c_in, c_out, n_src, E, seed):
    """x (signed: the first layer's features are), edge attributes and the layer's parameters with rows far apart in magnitude (the per-row, per-edge and
    per-matrix power-of-two scales of the fp16 forms)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_src, c_in, generator=g)
    x[::37] *= 50.0
    ea = torch.randn(E, FE, generator=g)
    ea[::29] *= 20.0
    We, be = torch.randn(c_in, FE, generator=g) * 0.3, torch.randn(c_in, generator=g)
    Wj, Wi, bj = torch.randn(c_out, c_in, generator=g) * 0.1, torch.randn(c_out, c_in, generator=g) * 0.1, torch.randn(c_out, generator=g)
    Wj[::7] *= 30.0
    scale, shift = torch.rand(c_out, generator=g) + 0.5, torch.randn(c_out, generator=g)
    return x, ea, We, be, Wj, bj, Wi, scale, shift


def decoder_inputs(seed, c=128):
    g = torch.Generator().manual_seed(seed)
    W0, b0 = torch.randn(64, c, generator=g) * 0.15, torch.randn(64, generator=g)
    s1, h1 = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    W3, b3 = torch.randn(2, 64, generator=g) * 0.3, torch.randn(2, generator=g)
    return W0, b0, s1, h1, W3, b3


# ---- tile geometry of the two-phase kernels ----------------------------------------------------------------------------------------------
def cin_pad(c_in):
    return 32 if c_in <= 32 else (64 if c_in <= 64 else 128)


def geometry(cp, c_out, family):
    """(TILE, TPW, grid_cap) from the sources' formulas.  fused.hip, FusedCfg / launch_fused: 8 waves, NSLICE = c_out / 32, RG = 8 / (2 NSLICE), TILE = 32 RG,
    TPW = TILE / 8, grid = min(ntiles, DGNN_NUM_CU).  fused_mfma.hip, Cfg2 / launch2: NW = 4 for cin_pad <= 64 except 64 -> 64, else 8; KS = 2 with 8 waves, else 1;
    RG = NW / (KS NSLICE), TILE = 32 RG, TPW = TILE / NW, grid = min(ntiles, DGNN_NUM_CU * (1 with 8 waves, 2 with 4))."""
    nslice = c_out // 32
    if family == "fused":
        nw, ks, per_cu = 8, 2, 1
    else:
        nw = 4 if (cp <= 64 and not (cp == 64 and c_out == 64)) else 8
        ks, per_cu = (2, 1) if nw == 8 else (1, 2)
    tile = 32 * (nw // (ks * nslice))
    return tile, tile // nw, NUM_CU * per_cu


TWO_PHASE = {            # (cin_pad, c_out, family): (TILE, TPW, grid_cap); geometry() gives the same (test_fused_layer_model_cpu.py)
    (32, 64, "fused"): (64, 8, 256), (64, 64, "fused"): (64, 8, 256),
    (32, 128, "fused"): (32, 4, 256), (64, 128, "fused"): (32, 4, 256), (128, 128, "fused"): (32, 4, 256),
    (32, 64, "mfma"): (64, 16, 512), (32, 128, "mfma"): (32, 8, 512), (64, 64, "mfma"): (64, 8, 256), (64, 128, "mfma"): (32, 8, 512),
    (128, 128, "mfma"): (32, 4, 256),
}
WS_GROUP = 4             # fused_ws.hip decides the path per group of four cells (tests/test_gpu_ws.py)


def deep_size(tile, grid_cap):
    return 4 * grid_cap * tile + tile + 9


def edge_sizes(tile, tpw, grid_cap):
    """destination counts to test one instantiation at: one cell, a group short of / past one cell, a tile and a cell, ten tiles with a ragged last one
    (workgroups with 0, 1 and 2 tiles in one launch) and the deep size (the pipelines of a workgroup run full: tiles_per_workgroup)"""
    return [1, tpw - 1, tpw + 1, tile + 1, 9 * tile + 9, deep_size(tile, grid_cap)]


def tiles_of_workgroups(n_dst, tile, grid_cap):
    """the kernels' XCD-aware tile -> workgroup map restated: a list (one entry per workgroup of the launch) of the tiles it walks, in its order.
    Workgroup b sits on XCD b & 7 in slot b >> 3; XCD x owns tiles [x per, (x + 1) per) with per = ceil(ntiles / 8) and its (nwg + 7 - x) >> 3 workgroups
    take them round robin."""
    ntiles = -(-n_dst // tile)
    nwg = max(1, min(ntiles, grid_cap))
    per = (ntiles + 7) // 8
    out = []
    for b in range(nwg):
        xcd, slot, wpx = b & 7, b >> 3, (nwg + 7 - (b & 7)) >> 3
        t_lo, t_hi = xcd * per, min(ntiles, (xcd + 1) * per)
        out.append(list(range(t_lo + slot, t_hi, wpx)) if t_lo + slot < t_hi else [])
    return out


def family_of(c_in, c_out, mode, ws_enabled=True, rows_16_byte=True):
    """the kernel a fused-layer call reaches (dgnn_sage_layer_fused_fwd / dgnn_sage_layer_fused_mfma_try): "fused", "mfma" or "ws".  rows_16_byte: the
    rows can be read in 16-byte pieces (stride a multiple of 4 floats, 16-byte aligned base)."""
    cp = cin_pad(c_in)
    nb = cp // 16
    if mode in ("f32", "bf16x3") or c_in % nb != 0 or (nb >= 4 and not rows_16_byte):
        return "fused"
    if mode == "f16x2" and c_in in (64, 128) and c_out == 128 and ws_enabled and rows_16_byte:
        return "ws"
    return "mfma"


# ---- the per-element check ---------------------------------------------------------------------------------------------------------------
def check_elements(out, ref, bound, deg=None, tpw=None):
    """|out - ref| <= bound element-wise -> (largest err / bound, None) when it holds, else (largest, report) with the worst (cell, column, err / bound),
    the number of elements outside, that cell's in-degree and whether its gather group of `tpw` cells was regular"""
    err = (out.double() - ref).abs()
    ratio = err / bound
    ratio[torch.isnan(ratio)] = float("inf")            # a NaN result is outside every bound
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst <= 1.0:
        return worst, None
    flat = int(ratio.argmax())
    cell, col = flat // ratio.size(1), flat % ratio.size(1)
    rep = {"cell": cell, "column": col, "err/bound": worst, "outside": int((ratio > 1.0).sum()), "cells_outside": int((ratio > 1.0).any(1).sum())}
    if deg is not None:
        rep["in_degree"] = int(deg[cell])
        if tpw is not None:
            rep["group_regular"] = bool(group_regular(deg, tpw)[cell])
    return worst, rep
