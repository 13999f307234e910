"""CPU-side model of the edge-filtered mean aggregation (dgnn_amd/csrc/aggregate.hip) for tests/test_aggregate_model_cpu.py and
tests/test_gpu_aggregate_edges.py: the file header of aggregate.hip restated in numpy, exact to the bit (`fmaf32`, `forward`, `backward`), the
host dispatch of agg_fwd_t / agg_bwd_t restated (`expected_kernel`: documentation of coverage, not an oracle), seeded graph builders whose plans
are stable sorts in numpy (independent of plan.hip), three input families and one table of cases.  No GPU import.

Arithmetic of the header, per (edge, channel), all in fp32:
  phi  = fmaf(We[c][f], A[e][f], phi) over f ascending, starting from be[c]   (fused filter) | phi[e][c] (given) | 1 (no filter)
  a    = (((0 + x*phi) + x*phi) + ...) / max(deg, 1)   multiply and add rounded separately, in-edges in plan order, IEEE division
  dm   = da[dst] / max(indeg(dst), 1);  dx = ((0 + dm*phi) + dm*phi) + ... over the source row's out-edges in ascending plan position,
         then one fadd of the addend for rows below n_add, then x > 0 ? dx : +0 (mask_dx);  dphi = dm * x (+ dphi_ext, one fadd)
  bf16 storage: inputs widened to fp32, outputs rounded to nearest-even bf16; `a` uses the unrounded fp32 phi even when phi is stored.
numpy's float32 multiply, add and divide are the IEEE operations (one ufunc call each: nothing is contracted); only fmaf has to be built.

Integer family.  x, phi | (We, A, be), the addend and k are drawn from {-3..3} \\ {0} and da[d] = indeg(d) * k: dm = k, every product and
partial sum is an integer, `family_inputs` asserts that the largest sum of absolute terms of the case stays below 2^24, so dWe / dbe are
exact in ANY summation order and equal the fp64 sums bit for bit: a dropped, doubled or foreign edge changes an integer.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

import gemm_model as gm

F32 = np.float32
NUM_CU = 256          # common.h: DGNN_NUM_CU
CH_ROWS = 16          # aggregate.hip
BWD_BLOCKS = 1024     # aggregate.hip: slabs of a fused backward at most
GRID_CAP = NUM_CU * 8  # common.h: dgnn_grid_cap(blocks, 8)
SWITCHES = ("DGNN_AGG_GROUPED", "DGNN_AGG_MFMA", "DGNN_AGG_BWD_NODX")


# ---- fp32 pieces ----------------------------------------------------------------------------------------------------------------------------
def bf16_round(a):
    """fp32 -> nearest-even bf16, returned as fp32 (NaN stays NaN)"""
    a = np.ascontiguousarray(a, dtype=F32)
    b = a.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(F32)
    return np.where(np.isnan(a), a, r).astype(F32)


_TIE_MASK, _TIE_HALF, _TINY = np.int64(0x1FFFFFFF), np.int64(0x10000000), 2.0 ** -125


def fmaf32(a, b, c):
    """fp32 fused multiply-add with ONE rounding, vectorised (finite values, no overflow).  The product of two fp32 values is exact in fp64.
    The sum s = fl64(p + c) is rounded once to fp64 and TwoSum gives its remainder.  float32(s) is the result unless s sits exactly half way
    between two fp32 neighbours while the remainder is not zero: then the remainder's sign decides, not the tie rule.  (If s is no such
    midpoint the exact sum lies on s's side of every midpoint, because midpoints are fp64 numbers and s is the fp64 number nearest to it.)
    In the normal fp32 range a midpoint is an fp64 number whose low 29 mantissa bits are 1 0...0; results below 2^-125 are checked by
    distance."""
    a, b, c = (np.asarray(t) for t in (a, b, c))
    if max(a.ndim, b.ndim, c.ndim) == 0:
        return fmaf32(a[None], b[None], c[None])[0]
    # (a, b given as float64 arrays are taken to hold fp32 values: filter_phi widens its operands once, not per attribute)
    wide = lambda t: t if t.dtype == np.float64 else t.astype(F32).astype(np.float64)
    with np.errstate(all="ignore"):
        p = wide(a) * wide(b)
        c64 = np.broadcast_to(c.astype(F32).astype(np.float64), p.shape)
        s = p + c64
        r = s.astype(F32)
        cand = ((np.ascontiguousarray(s).view(np.int64) & _TIE_MASK) == _TIE_HALF) | ((np.abs(s) < _TINY) & (s != 0))
        if cand.any():
            idx = np.nonzero(cand)
            ps, cs, ss, rs = p[idx], c64[idx], s[idx], r[idx]
            bb = ss - ps
            err = (ps - (ss - bb)) + (cs - bb)                    # TwoSum: ps + cs = ss + err exactly
            up = ss > rs.astype(np.float64)
            other = np.nextafter(rs, np.where(up, F32(np.inf), F32(-np.inf)).astype(F32))
            tie = np.abs(ss - rs.astype(np.float64)) == np.abs(other.astype(np.float64) - ss)
            toward_other = np.where(up, err > 0, err < 0)
            r = r.copy()
            r[idx] = np.where(tie & (err != 0) & toward_other & (ss != rs.astype(np.float64)), other, rs)
    return r


def filter_phi(ea, We, be):
    """phi [E, c] of the fused filter: the fmaf chain from be over the attributes in ascending order"""
    E, c = ea.shape[0], We.shape[0]
    phi = np.empty((E, c), F32)
    We64, ea64 = We.astype(np.float64), ea.astype(np.float64)
    step = max(1, 65536 // c)                                   # blocks of rows that stay in the cache through the chain
    for r0 in range(0, E, step):
        blk = np.broadcast_to(be[None, :], (min(step, E - r0), c))
        for f in range(We.shape[1]):
            blk = fmaf32(We64[None, :, f], ea64[r0:r0 + step, f, None], blk)
        phi[r0:r0 + step] = blk
    return phi


Filter = namedtuple("Filter", "ea We be")


def _stored(t, bf16):
    return None if t is None else (bf16_round(t) if bf16 else np.asarray(t, F32))


def forward(rowptr, src, eid, x, filter=None, phi=None, bf16=False):
    """-> (a [n_dst, c], phi [E_rows, c] | None).  eid None: the identity.  filter: Filter(ea, We, be); phi: given; neither: plain x.
    The returned phi (fused filter only) holds every row of ea, as stored (rounded to bf16 in bf16 storage)."""
    x, phi = _stored(x, bf16), _stored(phi, bf16)
    n_dst, c = rowptr.size - 1, x.shape[1]
    eid = np.arange(src.size, dtype=np.int64) if eid is None else eid.astype(np.int64)
    phi_out = None
    if filter is not None:
        phi = filter_phi(*filter)
        phi_out = bf16_round(phi) if bf16 else phi
    deg = np.diff(rowptr).astype(np.int64)
    acc = np.zeros((n_dst, c), F32)
    with np.errstate(all="ignore"):
        for t in range(int(deg.max()) if n_dst else 0):
            rows = np.nonzero(deg > t)[0]
            k = rowptr[rows].astype(np.int64) + t
            term = x[src[k]] if phi is None else x[src[k]] * phi[eid[k]]
            acc[rows] = acc[rows] + term
        a = acc / np.maximum(deg, 1).astype(F32)[:, None]
    return (bf16_round(a) if bf16 else a), phi_out


Bwd = namedtuple("Bwd", "dx dphi dWe dbe magW magb seqW seqb")


def backward(t_rowptr, t_dst, t_eid, rowptr_dst, x, da, filter=None, phi=None, add=None, n_add=0, dphi_ext=None, mask_dx=False, bf16=False,
             dphi_init=None, seq32=True):
    """-> Bwd.  dx [n_src, c]; dphi [rows of phi, c]: dphi_init (the caller's buffer, NaN if not given) with the plan's edges written;
    dWe / dbe: fp64 sums of the products dphi * A and of dphi (the fp32 dphi, before any dphi_ext), magW / magb their magnitude sums, seqW /
    seqb the same sums in fp32 in transposed-plan order with fmaf32 (a plain add for dbe) -- None without a fused filter or with seq32=False."""
    x, da, phi, add, dphi_ext = (_stored(t, bf16) for t in (x, da, phi, add, dphi_ext))
    n_src, c = t_rowptr.size - 1, x.shape[1]
    t_eid = t_eid.astype(np.int64)
    if filter is not None:
        phi = filter_phi(*filter)
    deg = np.diff(t_rowptr).astype(np.int64)
    row_of = np.repeat(np.arange(n_src), deg)
    cnt = np.maximum(np.diff(rowptr_dst), 1).astype(F32)
    with np.errstate(all="ignore"):
        dm = da[t_dst] / cnt[t_dst][:, None]                      # [E, c] in transposed-plan order
        dphi_k = dm * x[row_of]
        acc = np.zeros((n_src, c), F32)
        for t in range(int(deg.max()) if n_src else 0):
            rows = np.nonzero(deg > t)[0]
            k = t_rowptr[rows].astype(np.int64) + t
            acc[rows] = acc[rows] + (dm[k] if phi is None else dm[k] * phi[t_eid[k]])
        if add is not None and n_add > 0:
            acc[:n_add] = acc[:n_add] + add[:n_add]
        if mask_dx:
            acc = np.where(x > 0, acc, F32(0.0)).astype(F32)
        dx = bf16_round(acc) if bf16 else acc
        dphi = None
        if filter is None and phi is not None:
            n_rows = phi.shape[0]
            dphi = np.full((n_rows, c), np.nan, F32) if dphi_init is None else np.array(dphi_init, F32)
            if n_rows:
                out = dphi_k if dphi_ext is None else dphi_k + dphi_ext[t_eid]
                dphi[t_eid] = bf16_round(out) if bf16 else out
    if filter is None:      # (no filter: nothing is written to dphi)
        return Bwd(dx, dphi, None, None, None, None, None, None)
    A = filter.ea[t_eid].astype(np.float64)
    d64 = dphi_k.astype(np.float64)
    dWe, magW = d64.T @ A, np.abs(d64).T @ np.abs(A)
    dbe, magb = d64.sum(0), np.abs(d64).sum(0)
    seqW = seqb = None
    if seq32:
        seqW, seqb = np.zeros((c, A.shape[1]), F32), np.zeros(c, F32)
        A32 = filter.ea[t_eid]
        for k in range(t_dst.size):
            seqW = fmaf32(dphi_k[k][:, None], A32[k][None, :], seqW)
            seqb = seqb + dphi_k[k]
    return Bwd(dx, None, dWe, dbe, magW, magb, seqW, seqb)


def wgrad_rho(b):
    """largest |seq32 - ref64| / magnitude of the model's own sequential fp32 sums: gemm_model.wgrad_bound(rho) is the kernels' bound"""
    rho = 0.0
    for seq, ref, mag in ((b.seqW, b.dWe, b.magW), (b.seqb, b.dbe, b.magb)):
        ok = mag > 0
        if ok.any():
            rho = max(rho, float((np.abs(seq.astype(np.float64) - ref)[ok] / mag[ok]).max()))
    return rho


# ---- the host side of aggregate.hip, restated ----------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def chunk_rows(n):
    """rows per wavefront chunk: cdiv(n, 256 CUs * 16 wavefronts), rounded up to a multiple of 4, inside [4, 16]"""
    r = (_cdiv(n, NUM_CU * 16) + 3) & ~3
    return min(max(r, 4), CH_ROWS)


def chunk_blocks(n, rows_per_wave):
    return _cdiv(_cdiv(n, rows_per_wave), 4)


def bwd_blocks(n, rows_per_wave):
    """workgroups (= slabs) of a fused backward"""
    return min(chunk_blocks(n, rows_per_wave), BWD_BLOCKS)


def passes(kernel, n):
    """how many trips of its grid-stride loop the busiest wavefront of `kernel` (name without template arguments, or k_agg_fwd_m2 / _m4) makes
    over n rows: rows per pass = wavefronts of the capped grid * rows per wavefront step."""
    if n == 0:
        return 0
    if kernel == "k_agg_fwd":                              # one destination per wavefront, dgnn_grid_cap(cdiv(n, 4), 8) workgroups of 4
        per, waves = 1, 4 * min(_cdiv(n, 4), GRID_CAP)
    elif kernel in ("k_agg_fwd_g", "k_agg_bwd_g"):         # chunk_grid(n, chunk_rows(n))
        per = chunk_rows(n)
        waves = 4 * min(chunk_blocks(n, per), GRID_CAP)
    elif kernel in ("k_agg_fwd_m2", "k_agg_fwd_m4"):       # chunk_grid(n, 32 / NBK)
        per = 16 if kernel.endswith("2") else 8
        waves = 4 * min(chunk_blocks(n, per), GRID_CAP)
    elif kernel == "k_agg_bwd_mm":                         # bwd_blocks(n, 16)
        per, waves = 16, 4 * bwd_blocks(n, 16)
    else:
        assert kernel == "k_agg_bwd_c", kernel             # bwd_blocks(n, chunk_rows(n))
        per = chunk_rows(n)
        waves = 4 * bwd_blocks(n, per)
    return _cdiv(_cdiv(n, per), waves)


def env_switches(env=None):
    import os
    env = os.environ if env is None else env
    return {s: not env.get(s, "1").startswith("0") for s in SWITCHES}


def rows_of(n, op):
    """op: None (an operand that is not there) or (offset of the first element from a 16-byte aligned address, leading dimension), in elements"""
    return op is None or (op[0] % n == 0 and op[1] % n == 0)


def expected_kernel(entry, bf16, form, c_in, ops, on=None, has_dx=True, mask_dx=False):
    """The kernel instantiation agg_fwd_t / agg_bwd_t launch.  entry: fwd | bwd; form: given | fused20 | fused2 | plain; ops: operand name ->
    (offset, ld) | None for x, a, phi, phi_out (fwd) and x, da, dx, phi, dphi, add, dphi_ext (bwd); on: the three switches."""
    on = on or {s: True for s in SWITCHES}
    T = "bf16" if bf16 else "f32"
    g = lambda k: ops.get(k)
    given, fused20 = form == "given", form == "fused20"
    FE = {"fused20": 20, "fused2": 2, "given": 0, "plain": -1}[form]
    G = 8 if c_in <= 32 else (16 if c_in <= 64 else 32)
    wide2 = c_in % 2 == 0 and (c_in > 64 or bf16)
    if entry == "fwd":
        if given and g("phi_out") is None and on["DGNN_AGG_GROUPED"] and c_in % 4 == 0 and c_in <= 128 and all(rows_of(4, g(k)) for k in ("x", "phi", "a")):
            return "k_agg_fwd_g<%d,%s>" % (G, T)
        vw = 2 if c_in <= 32 else 4
        if not bf16 and on["DGNN_AGG_MFMA"] and fused20 and g("phi_out") is None and c_in <= 64 and c_in % vw == 0 and rows_of(vw, g("x")) and rows_of(vw, g("a")):
            return "k_agg_fwd_m<%d>" % vw
        v2 = wide2 and rows_of(2, g("x")) and rows_of(2, g("a")) and (not given or rows_of(2, g("phi"))) and rows_of(2, g("phi_out"))
        return "k_agg_fwd<%d,%d,%s>" % (2 if v2 else 1, FE, T)
    assert entry == "bwd"
    add = g("add") is not None
    if given and on["DGNN_AGG_GROUPED"] and g("dphi_ext") is None and c_in % 4 == 0 and c_in <= 128 and \
            all(rows_of(4, g(k)) for k in ("x", "phi", "da", "dx", "dphi", "add")):
        return "k_agg_bwd_g<%d,%s,%s>" % (G, T, "ADD" if add else "-")
    if not bf16 and on["DGNN_AGG_MFMA"] and fused20 and c_in <= 32 and c_in % 2 == 0 and not mask_dx and g("dphi") is None and \
            all(rows_of(2, g(k)) for k in ("x", "da", "dx", "add")):
        return "k_agg_bwd_mm<%s,%s>" % (("DX", "ADD" if add else "-") if has_dx else ("-", "-"))
    v2 = wide2 and all(rows_of(2, g(k)) for k in ("x", "da", "dx", "dphi")) and (not given or rows_of(2, g("phi")))
    cpl = 2 if v2 else 1
    slots = 4 if (cpl == 2 and not bf16) else 8
    if add and FE in (20, 0):
        tail = "ADD,DX"
    elif FE == 20 and not has_dx and on["DGNN_AGG_BWD_NODX"]:
        tail = "-,-"
    else:
        tail = "-,DX"
    return "k_agg_bwd_c<%d,%d,%s,%d,%s>" % (cpl, FE, T, slots, tail)


# every instantiation the two dispatch functions can choose (test_aggregate_model_cpu.py: CASES reaches each under the default switches)
def all_instantiations():
    out = set()
    for T in ("f32", "bf16"):
        out |= {"k_agg_fwd<%d,%d,%s>" % (cpl, fe, T) for cpl in (1, 2) for fe in (20, 2, 0, -1)}
        out |= {"k_agg_fwd_g<%d,%s>" % (G, T) for G in (8, 16, 32)}
        out |= {"k_agg_bwd_g<%d,%s,%s>" % (G, T, a) for G in (8, 16, 32) for a in ("ADD", "-")}
        for cpl in (1, 2):
            slots = 4 if (cpl == 2 and T == "f32") else 8
            out |= {"k_agg_bwd_c<%d,%d,%s,%d,-,DX>" % (cpl, fe, T, slots) for fe in (20, 2, 0, -1)}
            out.add("k_agg_bwd_c<%d,0,%s,%d,ADD,DX>" % (cpl, T, slots))         # given phi + addend: both storages (dgnn_sage_aggregate_bwd_phi_add)
            out.add("k_agg_bwd_c<%d,20,%s,%d,-,->" % (cpl, T, slots))           # no dx
    out |= {"k_agg_bwd_c<1,20,f32,8,ADD,DX>", "k_agg_bwd_c<2,20,f32,4,ADD,DX>"}  # fused + addend: fp32 only (dgnn_sage_aggregate_bwd_add)
    out |= {"k_agg_fwd_m<2>", "k_agg_fwd_m<4>", "k_agg_bwd_mm<DX,ADD>", "k_agg_bwd_mm<DX,->", "k_agg_bwd_mm<-,->"}
    return out


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------------
# ei [2, E_rows]: (source, destination) of every row of the edge arrays (phi, edge attributes, dphi); keep: which rows are edges of the plan --
# the others are rows the kernels must neither read nor write.
Graph = namedtuple("Graph", "n_src n_dst ei keep")
Plans = namedtuple("Plans", "rowptr src eid t_rowptr t_dst t_eid")


def plan_by(key, other, ids, n_key):
    """CSR of a stable sort by key: (rowptr, other, edge id), int32"""
    order = np.argsort(key, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n_key))])
    return rowptr.astype(np.int32), other[order].astype(np.int32), ids[order].astype(np.int32)


def plans(g):
    ids = np.nonzero(g.keep)[0]
    s, d = g.ei[0][ids], g.ei[1][ids]
    return Plans(*plan_by(d, s, ids, g.n_dst), *plan_by(s, d, ids, g.n_src))


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def tets(n, seed=0):
    """4-regular in both directions, in the reference layout (rows grouped by source, 4 each): a relabelled circulant i -> i +- 1, i +- s
    (a multigraph with self loops below 5 rows)"""
    r = _rng(1, n, seed)
    perm = r.permutation(n)
    s = max(2, int(round(n ** 0.5)))
    i = np.arange(n)
    nb = np.stack([(i + 1) % n, (i - 1) % n, (i + s) % n, (i - s) % n], 1)
    nb = np.take_along_axis(nb, np.argsort(r.random((n, 4)), 1), 1)
    ei = np.empty((2, 4 * n), np.int64)
    ei[0] = np.repeat(np.arange(n), 4)
    ei[1, perm[np.repeat(i, 4)] * 4 + np.tile(np.arange(4), n)] = perm[nb.reshape(-1)]
    return Graph(n, n, ei, np.ones(4 * n, bool))


def thinned(n, seed=0):
    """tets with 3 of 10 edges outside the plan: degrees 0..4 both ways (in-degrees of 3: the division), rows of the edge arrays that are no
    edges.  From 64 rows on it has rows of every degree 0..4, destinations with 3 in-edges and no edge at its last source row"""
    g = tets(n, seed)
    keep = _rng(2, n, seed).random(4 * n) < 0.7
    if n >= 64:
        keep[g.ei[0] == n - 1] = False
        keep[g.ei[0] == 0] = True
    g = g._replace(keep=keep)
    if n >= 64:
        od = np.bincount(g.ei[0][keep], minlength=n)
        idg = np.bincount(g.ei[1][keep], minlength=n)
        assert set(od) == {0, 1, 2, 3, 4} and (idg == 3).any() and (idg == 0).any()
    return g


def ragged(n_src, n_dst, seed=0):
    """hubs: sources with exactly 64, 65 and 130 out-edges (130: three 64-position windows of k_agg_bwd_c whatever the chunk's first position), a
    destination with exactly 130 in-edges, the others 0..6 out-edges; the list is shuffled, three rows of the edge arrays are no edges"""
    assert n_src >= 8 and n_dst >= 8
    r = _rng(3, n_src, n_dst, seed)
    hubs = {1: 64, n_src // 2: 65, n_src - 2: 130}
    hub_dst = n_dst // 3
    other_dst = np.setdiff1d(np.arange(n_dst), [hub_dst])
    other_src = np.setdiff1d(np.arange(n_src), list(hubs) + [0, n_src - 1])
    deg = r.integers(0, 7, n_src)
    deg[[0, n_src - 1]] = 0
    for h, k in hubs.items():
        deg[h] = k
    s = np.repeat(np.arange(n_src), deg)
    d = other_dst[r.integers(0, other_dst.size, s.size)]
    s = np.concatenate([s, other_src[r.integers(0, other_src.size, 130)], [0, 0, 0]])
    d = np.concatenate([d, np.full(130, hub_dst), [0, 0, 0]])
    keep = np.ones(s.size, bool)
    keep[-3:] = False
    p = r.permutation(s.size)
    g = Graph(n_src, n_dst, np.stack([s[p], d[p]]), keep[p])
    od = np.bincount(g.ei[0][g.keep], minlength=n_src)
    assert all(od[h] == k for h, k in hubs.items()) and np.bincount(g.ei[1][g.keep], minlength=n_dst)[hub_dst] == 130
    return g


def chunk64_degrees(rw, n):
    """key-row degrees: consecutive chunks of rw rows whose edge totals are 63, 64, 65, 64 (in the last row) and 65 (in the first row); every further whole
    chunk 4 per row, the last three rows (0, 5, 0)"""
    q = 64 // rw
    pats = [[q] * (rw - 1) + [q - 1], [q] * rw, [q] * (rw - 1) + [q + 1], [0] * (rw - 1) + [64], [65] + [0] * (rw - 1)]
    deg = np.full(n, 4, np.int64)
    assert n >= 5 * rw + 3 and chunk_rows(n) == rw
    deg[:5 * rw] = np.concatenate(pats)
    deg[-3:] = [0, 5, 0]
    return deg


def chunk64(n, side, seed=0):
    """the degrees of chunk64_degrees on the plan that the kernel under test walks -- side 'dst': in-degrees (forward), 'src': out-degrees
    (backward) --, random other ends, the list shuffled"""
    r = _rng(4, n, seed)
    key = np.repeat(np.arange(n), chunk64_degrees(chunk_rows(n), n))
    oth = r.integers(0, n, key.size)
    p = r.permutation(key.size)
    ei = np.stack([oth[p], key[p]]) if side == "dst" else np.stack([key[p], oth[p]])
    return Graph(n, n, ei, np.ones(key.size, bool))


def empty(n_src, n_dst):
    return Graph(n_src, n_dst, np.zeros((2, 0), np.int64), np.zeros(0, bool))


def grouped_by_dst(g):
    """the same edges listed by destination, every row an edge: the forward plan is the identity (eid NULL)"""
    ids = np.nonzero(g.keep)[0]
    o = ids[np.argsort(g.ei[1][ids], kind="stable")]
    return Graph(g.n_src, g.n_dst, g.ei[:, o], np.ones(o.size, bool))


def build_graph(case, side):
    """side: 'dst' for the forward, 'src' for the backward (chunk64 puts its degrees there)"""
    if case.graph == "tets":
        g = tets(case.n_src)
    elif case.graph == "thinned":
        g = thinned(case.n_src)
    elif case.graph == "ragged":
        g = ragged(case.n_src, case.n_dst)
    elif case.graph == "chunk64":
        g = chunk64(case.n_src, side)
    else:
        assert case.graph == "empty", case.graph
        g = empty(case.n_src, case.n_dst)
    assert (g.n_src, g.n_dst) == (case.n_src, case.n_dst)
    return grouped_by_dst(g) if "eid_none" in case.opts else g


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
Inputs = namedtuple("Inputs", "x da phi filter add dphi_ext")


def _ints(shape, gen):
    return gm.ints(shape, gen).numpy().astype(F32)


def family_inputs(case, g, seed=0):
    """x [n_src, c], da [n_dst, c], phi [E_rows, c] (given) | Filter (fused), add [n_src, c], dphi_ext [E_rows, c]; fp32, and bf16 values where the
    case's storage is bf16 (the filter stays fp32).  randn; wide: randn * 2^e, e per row from -8..8; integer: see the module docstring."""
    gen = torch.Generator().manual_seed((seed * 1000003 + case.c_in * 7919 + case.n_src * 31 + case.n_dst) % (2 ** 31))
    c, fe, E = case.c_in, {"fused20": 20, "fused2": 2}.get(case.form, 0), g.ei.shape[1]
    shapes = dict(x=(g.n_src, c), da=(g.n_dst, c), phi=(E, c), add=(g.n_src, c), ext=(E, c), ea=(E, fe), We=(c, fe), be=(c,))
    if case.family == "integer":
        v = {k: _ints(s, gen) for k, s in shapes.items()}
        keep_dst = g.ei[1][g.keep]
        indeg = np.maximum(np.bincount(keep_dst, minlength=g.n_dst), 1)
        if case.bf16:       # indeg * k must be a bf16 number: at most 8 significant bits
            v["da"] = np.where(np.abs(v["da"]) == 3, F32(1), v["da"])
        v["da"] = (v["da"] * indeg[:, None]).astype(F32)
        assert not case.bf16 or np.array_equal(bf16_round(v["da"]), v["da"])
        # the largest sums of absolute terms: |phi| <= 3 + 9 fe, a dx row 3 |phi| maxdeg + 3, a column of dWe 27 E
        n_e = int(g.keep.sum())
        maxdeg = max(int(np.bincount(g.ei[0][g.keep], minlength=1).max()), int(np.bincount(keep_dst, minlength=1).max())) if n_e else 0
        assert max(27 * n_e, 9 * (3 + 9 * fe) * maxdeg + 3) < 2 ** 24, "integer family: a sum could leave the exact range"
    else:
        v = {k: torch.randn(s, generator=gen).numpy().astype(F32) for k, s in shapes.items()}
        v["We"] *= F32(0.3)
        if case.family == "wide":
            for k in ("x", "da", "phi", "add", "ext"):
                e = torch.randint(-8, 9, (shapes[k][0], 1), generator=gen).numpy().astype(F32)
                v[k] = (v[k] * np.exp2(e)).astype(F32)
        else:
            assert case.family == "randn", case.family
    if case.bf16:
        for k in ("x", "da", "phi", "add", "ext"):
            v[k] = bf16_round(v[k])
    filt = Filter(v["ea"], v["We"], v["be"]) if fe else None
    return Inputs(v["x"], v["da"], v["phi"] if case.form == "given" else None, filt, v["add"], v["ext"])


# ---- the case table ------------------------------------------------------------------------------------------------------------------------------
# Thresholds, from the constants above (DGNN_NUM_CU = 256, dgnn_grid_cap(.., 8) = 2048 workgroups of 4 wavefronts, BWD_BLOCKS = 1024, CH_ROWS = 16):
#   chunk_rows(n) = clamp(roundup4(cdiv(n, 4096)), 4, 16): 4 up to 16384 rows, 8 up to 32768, 12 up to 49152, 16 from 49153.
#   k_agg_fwd: 2048 * 4 wavefronts, a destination each: 8192 per pass; 8193 takes a second pass.
#   k_agg_fwd_g / k_agg_bwd_g: 2048 * 4 chunks per pass; the cap only binds with 16-row chunks (4-, 8- and 12-row chunks end at 4096 chunks):
#       131072 rows per pass.  k_agg_fwd_m<2>: 8192 steps of 16 rows = 131072; k_agg_fwd_m<4>: 8192 steps of 8 rows = 65536.
#   k_agg_bwd_c / k_agg_bwd_mm: 1024 * 4 chunks / steps of 16 rows = 65536 rows per pass (again only with 16-row chunks).
#   so 65541 rows: 2 passes of bwd_c, bwd_mm, fwd_m<4>; 131093 rows: 3 passes of those (their wavefronts' third step: the matrix-core pair's
#   pipeline, rows requested two steps ahead, runs to its end) and 2 of fwd_m<2> and the _g pair.
#   k_reduce_slabs sums 1024 slabs when cdiv(cdiv(n, rw), 4) >= 1024: with 4-row chunks from 16369 rows (16384: 4096 chunks, exactly 1024), with
#   16-row chunks and in k_agg_bwd_mm from 65473 rows; 16385 rows (8-row chunks) fall back to 513 slabs.
# test_aggregate_model_cpu.py asserts all of this through `passes`, `chunk_rows` and `bwd_blocks`.
#
# align: al = every operand 16-byte aligned with a leading dimension that is a multiple of 4 | p1 = first element off by one element | ld2 = leading
# dimension a multiple of 2, not of 4 | ldodd = an odd leading dimension.  lde: leading dimension of the edge attributes (20 packed, 23 not).
# opts: phi_out, eid_none (fwd); no_dx, no_dphi (bwd); add, ext, mask (bwd_phi); n_add0 / n_add_all (addend forms: else n_add = min(n_src, n_dst) - 1).
Case = namedtuple("Case", "kernel entry bf16 form c_in graph n_src n_dst family align lde opts")
SIZES_SMALL = (1, 2, 3, 4, 5, 15, 16, 17, 33)
SIZES_LARGE = (16384, 16385, 32769, 49153, 65541, 131093)


def _case(kernel, entry, bf16, form, c_in, graph="thinned", n=257, n_dst=None, family="randn", align="al", lde=20, opts=()):
    return Case(kernel, entry, bool(bf16), form, c_in, graph, n, n if n_dst is None else n_dst, family, align, lde, tuple(opts))


def _build_cases():
    C, rows = _case, []
    fam = ("randn", "wide", "integer")
    # ---- forward -----------------------------------------------------------------------------------------------------------------------------
    for i, (c, G) in enumerate([(4, 8), (8, 8), (28, 8), (32, 8), (36, 16), (60, 16), (64, 16), (68, 32), (124, 32), (128, 32)]):
        rows.append(C("k_agg_fwd_g<%d>" % G, "fwd", i % 2, "given", c, ("thinned", "ragged")[i % 2], 257, 100 if i % 2 else None, fam[i % 3]))
    for bf in (0, 1):
        rows += [C("k_agg_fwd<2,0>", "fwd", bf, "given", 132, "ragged", 90, 300, "randn"), C("k_agg_fwd<2,0>", "fwd", bf, "given", 200, "thinned", 65, None, "wide"),
                 C("k_agg_fwd<1,0>", "fwd", bf, "given", 129, "thinned", 65, None, "integer"), C("k_agg_fwd<1,0>", "fwd", bf, "given", 1, "ragged", 40, 33, "randn"),
                 C("k_agg_fwd<1,0>", "fwd", bf, "given", 32, "thinned", 65, None, "randn", "p1"), C("k_agg_fwd<%d,0>" % (2 if bf else 1), "fwd", bf, "given", 32, "thinned", 65, None, "wide", "ld2"),
                 C("k_agg_fwd<1,0>", "fwd", bf, "given", 28, "ragged", 50, 50, "integer", "ldodd"), C("k_agg_fwd<2,0>", "fwd", bf, "given", 132, "thinned", 65, None, "integer", "ld2"),
                 C("k_agg_fwd<1,0>", "fwd", bf, "given", 132, "thinned", 65, None, "randn", "p1")]
    for i, c in enumerate((2, 6, 30, 32)):
        rows.append(C("k_agg_fwd_m<2>", "fwd", 0, "fused20", c, ("thinned", "tets", "ragged", "thinned")[i], 257, None, fam[i % 3], "al", (20, 23)[i % 2]))
    for i, c in enumerate((36, 60, 64)):
        rows.append(C("k_agg_fwd_m<4>", "fwd", 0, "fused20", c, ("thinned", "ragged", "tets")[i], 129, None, fam[i % 3], "al", (23, 20)[i % 2]))
    rows += [C("k_agg_fwd_m<2>", "fwd", 0, "fused20", 30, "thinned", 129, None, "randn", "ld2"), C("k_agg_fwd<1,20>", "fwd", 0, "fused20", 34, "thinned", 129, None, "randn"), C("k_agg_fwd<1,20>", "fwd", 0, "fused20", 34, "thinned", 129, None, "wide", "ldodd"),
             C("k_agg_fwd<1,20>", "fwd", 0, "fused20", 36, "thinned", 129, None, "randn", "ld2"), C("k_agg_fwd<1,20>", "fwd", 0, "fused20", 30, "ragged", 64, 70, "randn", "p1", 23),
             C("k_agg_fwd<2,20>", "fwd", 0, "fused20", 66, "thinned", 65, None, "randn"), C("k_agg_fwd<1,20>", "fwd", 0, "fused20", 65, "thinned", 65, None, "wide"),
             C("k_agg_fwd<2,20>", "fwd", 0, "fused20", 128, "ragged", 40, 33, "integer"), C("k_agg_fwd<2,20>", "fwd", 0, "fused20", 130, "thinned", 65, None, "randn", "ld2", 23),
             C("k_agg_fwd<1,20>", "fwd", 0, "fused20", 129, "thinned", 65, None, "randn"), C("k_agg_fwd<1,20>", "fwd", 0, "fused20", 1, "ragged", 40, 33, "wide"),
             C("k_agg_fwd<1,20>", "fwd", 0, "fused20", 32, "thinned", 129, None, "randn", "al", 20, ("phi_out",)), C("k_agg_fwd<2,20>", "fwd", 0, "fused20", 130, "thinned", 65, None, "wide", "al", 20, ("phi_out",)),
             C("k_agg_fwd<1,20>", "fwd", 0, "fused20", 130, "thinned", 65, None, "randn", "p1")]
    rows += [C("k_agg_fwd<2,20>", "fwd", 1, "fused20", c, g, n, nd, f, al, lde, o) for c, g, n, nd, f, al, lde, o in
             [(2, "thinned", 129, None, "randn", "al", 20, ()), (64, "ragged", 40, 33, "integer", "al", 23, ()), (130, "thinned", 65, None, "wide", "ld2", 20, ()),
              (36, "thinned", 129, None, "randn", "al", 20, ("phi_out",))]]
    rows += [C("k_agg_fwd<1,20>", "fwd", 1, "fused20", c, "thinned", 65, None, f, al, 20, o) for c, f, al, o in
             [(65, "randn", "al", ()), (1, "wide", "al", ()), (30, "randn", "p1", ("phi_out",)), (30, "integer", "ldodd", ())]]
    for bf in (0, 1):
        rows += [C("k_agg_fwd<1,2>", "fwd", bf, "fused2", 1, "thinned", 65, None, "randn", "al", 2), C("k_agg_fwd<%d,2>" % (2 if bf else 1), "fwd", bf, "fused2", 48, "ragged", 40, 33, "integer", "al", 5),
                 C("k_agg_fwd<2,2>", "fwd", bf, "fused2", 130, "thinned", 65, None, "wide", "al", 2, ("phi_out",)),
                 C("k_agg_fwd<1,-1>", "fwd", bf, "plain", 1, "thinned", 65, None, "randn"), C("k_agg_fwd<%d,-1>" % (2 if bf else 1), "fwd", bf, "plain", 28, "ragged", 40, 33, "integer"),
                 C("k_agg_fwd<2,-1>", "fwd", bf, "plain", 130, "thinned", 65, None, "wide")]
    # eid NULL on a destination-grouped list: every forward kernel
    rows += [C("k_agg_fwd_g<8>", "fwd", 0, "given", 4, "ragged", 64, 70, "randn", "al", 20, ("eid_none",)), C("k_agg_fwd_m<2>", "fwd", 0, "fused20", 2, "thinned", 129, None, "randn", "al", 20, ("eid_none",)),
             C("k_agg_fwd_m<4>", "fwd", 0, "fused20", 36, "ragged", 64, 70, "randn", "al", 20, ("eid_none",)), C("k_agg_fwd<1,20>", "fwd", 0, "fused20", 1, "ragged", 64, 70, "randn", "al", 20, ("eid_none", "phi_out")),
             C("k_agg_fwd<1,-1>", "fwd", 0, "plain", 1, "thinned", 129, None, "randn", "al", 20, ("eid_none",))]
    # sizes, each kernel at its narrowest width; chunk64: the chunk totals 63 / 64 / 65 of the lane-group kernels
    for i, n in enumerate(SIZES_SMALL):       # two of the four kernels per size, every kernel at 1, 4, 5, 16, 17 or at 2, 3, 15, 33 and at one more
        four = [C("k_agg_fwd_g<8>", "fwd", n % 2, "given", 4, "tets", n), C("k_agg_fwd_m<2>", "fwd", 0, "fused20", 2, "tets", n), C("k_agg_fwd_m<4>", "fwd", 0, "fused20", 36, "tets", n),
                C("k_agg_fwd<1,0>", "fwd", n % 2, "given", 1, "tets", n)]
        rows += four if n in (1, 17) else four[i % 2::2]
    rows += [C("k_agg_fwd_g<8>", "fwd", 0, "given", 4, "chunk64", 23), C("k_agg_fwd_g<8>", "fwd", 1, "given", 4, "chunk64", 49153), C("k_agg_fwd_g<16>", "fwd", 0, "given", 36, "chunk64", 23),
             C("k_agg_fwd_g<32>", "fwd", 1, "given", 68, "chunk64", 23), C("k_agg_fwd_g<8>", "fwd", 0, "given", 4, "empty", 9, 7), C("k_agg_fwd_m<2>", "fwd", 0, "fused20", 2, "empty", 9, 7),
             C("k_agg_fwd<1,-1>", "fwd", 1, "plain", 1, "empty", 9, 7)]
    for n in SIZES_LARGE:
        rows += [C("k_agg_fwd_g<8>", "fwd", 0, "given", 4, "thinned" if n == 32769 else "tets", n)]
    rows += [C("k_agg_fwd_g<16>", "fwd", 1, "given", 36, "tets", 131093), C("k_agg_fwd_g<32>", "fwd", 0, "given", 68, "tets", 131093),
             C("k_agg_fwd_m<2>", "fwd", 0, "fused20", 2, "tets", 65541), C("k_agg_fwd_m<2>", "fwd", 0, "fused20", 2, "thinned", 131093),
             C("k_agg_fwd_m<4>", "fwd", 0, "fused20", 36, "tets", 65541), C("k_agg_fwd_m<4>", "fwd", 0, "fused20", 36, "tets", 131093),
             C("k_agg_fwd<1,0>", "fwd", 0, "given", 1, "tets", 16385), C("k_agg_fwd<2,-1>", "fwd", 1, "plain", 2, "thinned", 16385),
             C("k_agg_fwd<1,20>", "fwd", 0, "fused20", 1, "tets", 8193)]
    # ---- backward: dgnn_sage_aggregate_bwd / _bf16 ----------------------------------------------------------------------------------------------------
    for i, (c, G) in enumerate([(4, 8), (8, 8), (28, 8), (32, 8), (36, 16), (60, 16), (64, 16), (68, 32), (124, 32), (128, 32)]):
        rows.append(C("k_agg_bwd_g<%d,->" % G, "bwd", (i + 1) % 2, "given", c, ("ragged", "thinned")[i % 2], 100 if i % 2 == 0 else 257, 257, fam[i % 3]))
    for bf in (0, 1):
        s2 = 8 if bf else 4
        rows += [C("k_agg_bwd_c<2,0,%d>" % s2, "bwd", bf, "given", 132, "ragged", 90, 300, "randn"), C("k_agg_bwd_c<2,0,%d>" % s2, "bwd", bf, "given", 200, "thinned", 65, None, "wide"),
                 C("k_agg_bwd_c<1,0,8>", "bwd", bf, "given", 129, "thinned", 65, None, "integer"), C("k_agg_bwd_c<1,0,8>", "bwd", bf, "given", 1, "ragged", 40, 33, "randn"),
                 C("k_agg_bwd_c<1,0,8>", "bwd", bf, "given", 32, "ragged", 65, 40, "randn", "p1"), C("k_agg_bwd_c<%d,0,8>" % (2 if bf else 1), "bwd", bf, "given", 32, "thinned", 65, None, "wide", "ld2"),
                 C("k_agg_bwd_c<1,0,8>", "bwd", bf, "given", 28, "ragged", 50, 50, "integer", "ldodd"), C("k_agg_bwd_c<2,0,%d>" % s2, "bwd", bf, "given", 132, "ragged", 65, 40, "integer", "ld2"),
                 C("k_agg_bwd_g<8,->", "bwd", bf, "given", 8, "thinned", 129, None, "randn", "al", 20, ("no_dx",)), C("k_agg_bwd_g<16,->", "bwd", bf, "given", 36, "ragged", 64, 70, "randn", "al", 20, ("no_dphi",)),
                 C("k_agg_bwd_c<1,0,8>", "bwd", bf, "given", 129, "ragged", 64, 70, "randn", "al", 20, ("no_dx",)),
                 # fused 2, no filter
                 C("k_agg_bwd_c<1,2,8>", "bwd", bf, "fused2", 1, "thinned", 65, None, "randn", "al", 2), C("k_agg_bwd_c<%d,2,8>" % (2 if bf else 1), "bwd", bf, "fused2", 48, "ragged", 40, 33, "integer", "al", 5),
                 C("k_agg_bwd_c<2,2,%d>" % s2, "bwd", bf, "fused2", 130, "ragged", 65, 40, "wide", "al", 2),
                 C("k_agg_bwd_c<1,-1,8>", "bwd", bf, "plain", 1, "thinned", 65, None, "randn"), C("k_agg_bwd_c<%d,-1,8>" % (2 if bf else 1), "bwd", bf, "plain", 28, "ragged", 40, 33, "integer"),
                 C("k_agg_bwd_c<2,-1,%d>" % s2, "bwd", bf, "plain", 130, "ragged", 65, 40, "wide")]
    for i, c in enumerate((2, 6, 30, 32)):
        rows.append(C("k_agg_bwd_mm<DX,->", "bwd", 0, "fused20", c, ("thinned", "tets", "ragged", "thinned")[i], 257, None, fam[i % 3], "al", (20, 23)[i % 2]))
        rows.append(C("k_agg_bwd_mm<-,->", "bwd", 0, "fused20", c, ("ragged", "thinned", "tets", "thinned")[i], 257, None, fam[(i + 1) % 3], "al", (23, 20)[i % 2], ("no_dx",)))
    rows += [C("k_agg_bwd_mm<DX,->", "bwd", 0, "fused20", 30, "thinned", 129, None, "randn", "ld2"), C("k_agg_bwd_c<1,20,8>", "bwd", 0, "fused20", 30, "thinned", 129, None, "wide", "ldodd"),
             C("k_agg_bwd_c<1,20,8>", "bwd", 0, "fused20", 32, "ragged", 64, 70, "randn", "p1", 23), C("k_agg_bwd_c<1,20,8>", "bwd", 0, "fused20", 34, "thinned", 129, None, "randn"),
             C("k_agg_bwd_c<1,20,8>", "bwd", 0, "fused20", 64, "ragged", 40, 33, "integer"), C("k_agg_bwd_c<1,20,8>", "bwd", 0, "fused20", 60, "thinned", 65, None, "wide", "al", 23),
             C("k_agg_bwd_c<2,20,4>", "bwd", 0, "fused20", 66, "thinned", 65, None, "randn"),
             C("k_agg_bwd_c<1,20,8>", "bwd", 0, "fused20", 65, "thinned", 65, None, "wide"), C("k_agg_bwd_c<2,20,4>", "bwd", 0, "fused20", 128, "ragged", 40, 33, "integer", "al", 23),
             C("k_agg_bwd_c<2,20,4>", "bwd", 0, "fused20", 130, "ragged", 65, 40, "randn", "ld2"), C("k_agg_bwd_c<1,20,8>", "bwd", 0, "fused20", 129, "thinned", 65, None, "randn"),
             C("k_agg_bwd_c<1,20,8>", "bwd", 0, "fused20", 1, "ragged", 40, 33, "wide"), C("k_agg_bwd_c<1,20,8,nodx>", "bwd", 0, "fused20", 1, "ragged", 40, 33, "randn", "al", 20, ("no_dx",)),
             C("k_agg_bwd_c<1,20,8,nodx>", "bwd", 0, "fused20", 36, "thinned", 129, None, "integer", "al", 23, ("no_dx",)), C("k_agg_bwd_c<2,20,4,nodx>", "bwd", 0, "fused20", 66, "ragged", 65, 40, "randn", "al", 20, ("no_dx",)),
             C("k_agg_bwd_c<1,20,8,nodx>", "bwd", 0, "fused20", 30, "thinned", 129, None, "randn", "p1", 20, ("no_dx",))]
    rows += [C("k_agg_bwd_c<%d,20,8%s>" % (cpl, ",nodx" if o else ""), "bwd", 1, "fused20", c, g, n, nd, f, al, lde, o) for cpl, c, g, n, nd, f, al, lde, o in
             [(2, 2, "thinned", 129, None, "randn", "al", 20, ()), (2, 64, "ragged", 40, 33, "integer", "al", 23, ()), (2, 130, "ragged", 65, 40, "wide", "ld2", 20, ()),
              (1, 65, "thinned", 65, None, "randn", "al", 20, ()), (1, 1, "ragged", 40, 33, "wide", "al", 20, ()), (1, 30, "thinned", 65, None, "integer", "ldodd", 20, ()),
              (2, 36, "thinned", 129, None, "randn", "al", 20, ("no_dx",)), (1, 29, "ragged", 65, 40, "randn", "al", 23, ("no_dx",))]]
    for i, n in enumerate(SIZES_SMALL):
        four = [C("k_agg_bwd_g<8,->", "bwd", n % 2, "given", 4, "tets", n), C("k_agg_bwd_mm<DX,->", "bwd", 0, "fused20", 2, "tets", n, None, "randn"),
                C("k_agg_bwd_c<1,20,8>", "bwd", 0, "fused20", 1, "tets", n, None, "integer"), C("k_agg_bwd_c<1,0,8>", "bwd", n % 2, "given", 1, "tets", n)]
        rows += four if n in (1, 17) else four[i % 2::2]
    rows += [C("k_agg_bwd_g<8,->", "bwd", 0, "given", 4, "chunk64", 23), C("k_agg_bwd_g<8,->", "bwd", 1, "given", 4, "chunk64", 49153), C("k_agg_bwd_g<16,->", "bwd", 1, "given", 36, "chunk64", 23),
             C("k_agg_bwd_g<32,->", "bwd", 0, "given", 68, "chunk64", 23), C("k_agg_bwd_c<1,0,8>", "bwd", 0, "given", 1, "chunk64", 23), C("k_agg_bwd_c<1,20,8>", "bwd", 0, "fused20", 1, "chunk64", 23, None, "integer"),
             C("k_agg_bwd_c<1,20,8>", "bwd", 0, "fused20", 1, "chunk64", 49153, None, "integer"), C("k_agg_bwd_mm<DX,->", "bwd", 0, "fused20", 2, "chunk64", 23, None, "randn"),
             C("k_agg_bwd_g<8,->", "bwd", 0, "given", 4, "empty", 9, 7), C("k_agg_bwd_mm<DX,->", "bwd", 0, "fused20", 2, "empty", 9, 7), C("k_agg_bwd_c<1,2,8>", "bwd", 1, "fused2", 1, "empty", 9, 7, "randn", "al", 2)]
    for n in SIZES_LARGE:
        g = "thinned" if n == 32769 else "tets"
        rows += [C("k_agg_bwd_g<8,->", "bwd", 0, "given", 4, g, n), C("k_agg_bwd_c<1,20,8>", "bwd", 0, "fused20", 1, g, n, None, "integer"), C("k_agg_bwd_mm<DX,->", "bwd", 0, "fused20", 2, g, n, None, "integer")]
    rows += [C("k_agg_bwd_g<8,->", "bwd", 1, "given", 4, "tets", 32769),      # a last chunk of 9 rows whose ninth has out-edges
             C("k_agg_bwd_g<16,->", "bwd", 1, "given", 36, "tets", 131093), C("k_agg_bwd_g<32,->", "bwd", 0, "given", 68, "tets", 131093),
             C("k_agg_bwd_mm<-,->", "bwd", 0, "fused20", 2, "thinned", 131093, None, "integer", "al", 20, ("no_dx",)),
             C("k_agg_bwd_c<1,0,8>", "bwd", 0, "given", 1, "tets", 131093), C("k_agg_bwd_c<2,20,8>", "bwd", 1, "fused20", 2, "tets", 131093, None, "integer"),
             C("k_agg_bwd_c<2,20,4>", "bwd", 0, "fused20", 66, "tets", 16384, None, "integer")]
    # ---- backward with the addend: dgnn_sage_aggregate_bwd_add (fused 20, fp32) ----------------------------------------------------------------------
    rows += [C("k_agg_bwd_mm<DX,ADD>", "bwd_add", 0, "fused20", 2, "thinned", 257, None, "randn"), C("k_agg_bwd_mm<DX,ADD>", "bwd_add", 0, "fused20", 30, "ragged", 100, 40, "wide", "al", 23),
             C("k_agg_bwd_mm<DX,ADD>", "bwd_add", 0, "fused20", 32, "ragged", 40, 100, "integer", "ld2"), C("k_agg_bwd_mm<DX,ADD>", "bwd_add", 0, "fused20", 6, "tets", 65, None, "randn", "al", 20, ("n_add0",)),
             C("k_agg_bwd_mm<DX,ADD>", "bwd_add", 0, "fused20", 6, "thinned", 65, None, "randn", "al", 20, ("n_add_all",)), C("k_agg_bwd_mm<DX,ADD>", "bwd_add", 0, "fused20", 2, "tets", 131093, None, "integer"),
             C("k_agg_bwd_c<1,20,8,ADD>", "bwd_add", 0, "fused20", 34, "thinned", 129, None, "randn"), C("k_agg_bwd_c<1,20,8,ADD>", "bwd_add", 0, "fused20", 1, "ragged", 100, 40, "wide"),
             C("k_agg_bwd_c<1,20,8,ADD>", "bwd_add", 0, "fused20", 30, "ragged", 40, 100, "integer", "ldodd"), C("k_agg_bwd_c<2,20,4,ADD>", "bwd_add", 0, "fused20", 66, "ragged", 100, 40, "randn"),
             C("k_agg_bwd_c<2,20,4,ADD>", "bwd_add", 0, "fused20", 130, "thinned", 65, None, "integer", "ld2", 23), C("k_agg_bwd_c<1,20,8,ADD>", "bwd_add", 0, "fused20", 65, "thinned", 65, None, "randn", "al", 20, ("n_add0",)),
             C("k_agg_bwd_c<2,20,4,ADD>", "bwd_add", 0, "fused20", 66, "thinned", 65, None, "randn", "al", 20, ("n_add_all",)), C("k_agg_bwd_c<1,20,8,ADD>", "bwd_add", 0, "fused20", 1, "chunk64", 49153, None, "integer"),
             C("k_agg_bwd_c<1,20,8,ADD>", "bwd_add", 0, "fused20", 1, "tets", 65541, None, "integer"), C("k_agg_bwd_c<1,20,8,ADD>", "bwd_add", 0, "fused20", 1, "chunk64", 23, None, "randn")]
    # ---- given phi with the addend, dphi_ext and the ReLU mask: dgnn_sage_aggregate_bwd_phi_add_masked --------------------------------------------------
    for i, (c, G) in enumerate([(4, 8), (36, 16), (68, 32)]):
        for bf in (0, 1):
            rows += [C("k_agg_bwd_g<%d,ADD>" % G, "bwd_phi", bf, "given", c, ("ragged", "thinned", "ragged")[i], (100, 257, 40)[i], (40, 257, 100)[i], fam[(i + bf) % 3], "al", 20, ("add", "mask")[:1 + (i + bf) % 2]),
                     C("k_agg_bwd_g<%d,->" % G, "bwd_phi", bf, "given", c, "thinned", 129, None, "randn", "al", 20, ("mask",))]
    for bf in (0, 1):
        s2 = 8 if bf else 4
        rows += [C("k_agg_bwd_c<%d,0,8,ADD>" % (2 if bf else 1), "bwd_phi", bf, "given", 4, "ragged", 100, 40, "randn", "al", 20, ("add", "ext")), C("k_agg_bwd_c<1,0,8,ADD>", "bwd_phi", bf, "given", 29, "thinned", 129, None, "wide", "al", 20, ("add", "mask")),
                 C("k_agg_bwd_c<2,0,%d,ADD>" % s2, "bwd_phi", bf, "given", 132, "ragged", 40, 100, "integer", "al", 20, ("add", "ext", "mask")), C("k_agg_bwd_c<2,0,%d,ADD>" % s2, "bwd_phi", bf, "given", 130, "thinned", 65, None, "randn", "ld2", 20, ("add", "n_add_all")),
                 C("k_agg_bwd_c<%d,0,8>" % (2 if bf else 1), "bwd_phi", bf, "given", 36, "thinned", 129, None, "randn", "al", 20, ("ext",)), C("k_agg_bwd_c<1,0,8,ADD>", "bwd_phi", bf, "given", 8, "thinned", 65, None, "randn", "p1", 20, ("add", "n_add0", "mask")),
                 C("k_agg_bwd_g<8,ADD>", "bwd_phi", bf, "given", 4, "chunk64", 23, None, "randn", "al", 20, ("add", "mask")), C("k_agg_bwd_c<1,0,8,ADD>", "bwd_phi", bf, "given", 1, "chunk64", 23, None, "integer", "al", 20, ("add", "ext", "mask"))]
    rows += [C("k_agg_bwd_g<8,ADD>", "bwd_phi", 0, "given", 4, "chunk64", 49153, None, "randn", "al", 20, ("add", "mask")), C("k_agg_bwd_g<8,ADD>", "bwd_phi", 1, "given", 4, "tets", 131093, None, "randn", "al", 20, ("add", "n_add_all")),
             C("k_agg_bwd_c<1,0,8,ADD>", "bwd_phi", 0, "given", 1, "chunk64", 49153, None, "randn", "al", 20, ("add", "ext", "mask")), C("k_agg_bwd_g<8,ADD>", "bwd_phi", 0, "given", 4, "empty", 9, 7, "randn", "al", 20, ("add", "mask"))]
    return rows


CASES = _build_cases()
ALIGN = {"al": (0, 0), "p1": (1, 0), "ld2": (0, 2), "ldodd": (0, 1)}     # (first element off 16-byte alignment, leading dimension mod 4), in elements


def case_id(c):
    return "%s-%s-%s-c%d-%s-%dx%d-%s-%s-e%d%s" % (c.entry, "bf16" if c.bf16 else "f32", c.form, c.c_in, c.graph, c.n_src, c.n_dst, c.family, c.align, c.lde,
                                                 "".join("-" + o for o in c.opts))


def n_add_of(case):
    if "n_add0" in case.opts:
        return 0
    return case.n_src if "n_add_all" in case.opts else max(min(case.n_src, case.n_dst) - 1, 0)


def leading_dim(cols, ld_mod4, before=3, after=2):
    """columns behind the row's last so that before + cols + after' = ld_mod4 (mod 4), after' >= after; an odd ld for ld_mod4 = 1"""
    return after + (ld_mod4 - (before + cols + after)) % 4


def case_operands(case):
    """operand name -> (offset, ld) | None, as expected_kernel takes them: every operand of a case shares the case's alignment"""
    off, m = ALIGN[case.align]
    o = case.opts
    op = (off, 3 + case.c_in + leading_dim(case.c_in, m))
    assert op[1] % 4 == m and op[1] >= case.c_in + 5
    given = case.form == "given"
    if case.entry == "fwd":
        return dict(x=op, a=op, phi=op if given else None, phi_out=op if "phi_out" in o else None)
    add = case.entry == "bwd_add" or "add" in o
    return dict(x=op, da=op, dx=None if "no_dx" in o else op, phi=op if given else None, dphi=op if given and "no_dphi" not in o else None,
                add=op if add else None, dphi_ext=op if "ext" in o else None)


def case_kernel(case, on=None):
    """expected_kernel of a case, and the short name its table row carries"""
    full = expected_kernel("fwd" if case.entry == "fwd" else "bwd", case.bf16, case.form, case.c_in, case_operands(case), on,
                           has_dx="no_dx" not in case.opts, mask_dx="mask" in case.opts)
    return full


def short_name(full):
    """k_agg_bwd_c<2,20,f32,4,ADD,DX> -> k_agg_bwd_c<2,20,4,ADD>: the table's spelling (storage is a column of its own)"""
    name, args = full[:-1].split("<")
    a = [t for t in args.split(",") if t not in ("f32", "bf16")]
    if name == "k_agg_bwd_c":
        tail = {("-", "DX"): [], ("ADD", "DX"): ["ADD"], ("-", "-"): ["nodx"]}[(a[3], a[4])]
        a = a[:3] + tail
    return "%s<%s>" % (name, ",".join(a))
