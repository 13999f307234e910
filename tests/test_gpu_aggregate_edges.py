"""Every kernel of dgnn_amd/csrc/aggregate.hip against tests/aggregate_model.py, the file header of aggregate.hip restated in numpy exact to the
bit (test_aggregate_model_cpu.py holds the model to exact rational arithmetic, the oracle's propagate_mean and fp64 autograd).  Calls go
through the C ABI; inputs sit in NaN-filled buffers, outputs in canary buffers, each with two spare rows, pad columns on both sides and the
case's alignment and leading dimension; rows of the edge arrays that are no edges of the plan hold NaN on the way in and must keep what
the caller left in the output.  Per case: return code 0, nothing written outside the outputs, a / phi_out / dx / dphi equal to the model bit for bit in both
storages, dWe / dbe equal to fp64 exactly in the integer family and within B = wgrad_bound(rho) of their magnitude sums otherwise (rho: the
error of the model's own sequential fp32 sums on the same inputs), a second call the same bits.  No assertion depends on which kernel ran: the
file passes unchanged under DGNN_AGG_GROUPED=0, DGNN_AGG_MFMA=0 and DGNN_AGG_BWD_NODX=0 DGNN_AGG_MFMA=0.

Reached under the default switches (aggregate_model.expected_kernel over CASES; test_aggregate_model_cpu.py asserts the list is complete):
  k_agg_fwd<CPL, FE, T>       CPL 1, 2 x FE 20, 2, 0, -1 x fp32, bf16; 2 and 3 passes of 8192 destinations (8193, 16385 rows)
  k_agg_fwd_g<G, T>           G 8, 16, 32 x fp32, bf16; chunks of 4, 8, 12 and 16 rows, chunk totals of 63 / 64 / 65 edges with 4- and 16-row
                              chunks, 2 passes (131093 rows)
  k_agg_fwd_m<NBK>            2 (2 passes at 131093 rows), 4 (2 passes at 65541, 3 at 131093: the index pipeline's third step)
  k_agg_bwd_g<G, T, ADD>      G 8, 16, 32 x fp32, bf16 x with / without the addend; the chunk sizes and totals of the forward, 2 passes
  k_agg_bwd_mm<DX, ADD>       <-,->, <DX,->, <DX,ADD>; 2 passes at 65541 rows, 3 at 131093; the per-edge path (ragged) and the division (thinned)
  k_agg_bwd_c<CPL, FE, T, SLOTS, ADD, DX>   the 26 instantiations of the dispatch; chunks of 4, 8, 12, 16 rows; 3 passes at 131093 rows; a row
                              across three 64-position windows (130 out-edges); the 16 parked addend rows (49153, 65541 rows)
  k_reduce_slabs              1024 slabs with 4-row chunks (16384 rows), 513 (16385), 1024 with 16-row chunks (65541, 131093)

Measured on an MI355X under the default switches, largest |dWe or dbe error| / (B * magnitude) per kernel over the randn and wide cases (B
between 2^-23 and 1.3e-6; the integer cases are exact):
  k_agg_bwd_c<1,20,8> 0.26   <1,20,8,ADD> 0.098   <1,20,8,nodx> 0.25   <2,20,4> 0.069   <2,20,4,ADD> 0.070   <2,20,4,nodx> 0.073
  k_agg_bwd_c<2,20,8> 0.067  <2,20,8,nodx> 0.081  <1,2,8> 0.087        <2,2,4> 0.084    <2,2,8> 0.098
  k_agg_bwd_mm<DX,-> 0.26    <DX,ADD> 0.20        <-,-> 0.090
(with DGNN_AGG_MFMA=0 the matrix-core cases run k_agg_bwd_c<1,20,8,ADD>: 0.14 there; every other figure is the same or smaller.)

Defects found, both fixed in aggregate.hip; on the kernels as they were, exactly the cases named here fail:
 1. k_agg_bwd_mm gave an empty edge slot dphi = 0 * x[row].  A source row with fewer than four out-edges that holds NaN or Inf in x therefore
    put NaN into dWe / dbe, which neither k_agg_bwd_c nor autograd over index_select does (they never read x for a slot without an edge).
    The slot's dphi is now 0 by selection; dx and the ordinary dWe / dbe bits are unchanged.  test_non_finite_rows_without_edges_stay_local
    (the three k_agg_bwd_mm cases on the thinned graph) holds every backward form to it.
 2. chunk_row (k_agg_fwd_g, k_agg_bwd_g) read rowptr[rc + 1] by a shuffle that only the lanes WITH a row executed.  The lane that holds it can
    belong to a group without a row -- 8-lane groups and a chunk of exactly 9 rows: row 8 reads lane 9, whose group would have row 9 -- and a
    lane that sits out hands out 0: the row's degree came out negative, its `a` / dx as 0 and its dphi unwritten.  9-row chunks only arise
    as the last chunk of 12- or 16-row chunks (from 32769 rows on), where no test looked: test_forward[...c4-thinned-32769x32769...] found
    it (the last destination has two in-edges).  Every lane now takes part in both shuffles.
"""

import numpy as np
import pytest
import torch

import aggregate_model as am
import gemm_model as gm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CANARY = -(2.0 ** 24)          # around every output; exact in fp32 and bf16
LEFT = -(2.0 ** 20)            # inside every output before the call: what the caller left there (no result of any case)
E_INVALID, E_UNSUPPORTED = -1, -2
ON = am.env_switches()
WORST = {}


def addr(t):
    """device address of a tensor (None -> NULL).  torch reports no address for a tensor without elements (E == 0): such a view still sits inside
    its buffer, and the entry points want a pointer there"""
    import ctypes
    if t is None:
        return None
    if t.numel() > 0:
        return ctypes.c_void_p(t.data_ptr())
    base = t._base
    assert base is not None and base.numel() > 0
    return ctypes.c_void_p(base.data_ptr() + (t.storage_offset() - base.storage_offset()) * t.element_size())


def _lib():
    from dgnn_amd._lib import lib, stream_ptr
    return lib(), addr, stream_ptr


def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def place(arr, case, fill, cols_ld=None):
    """arr [rows, cols] on the device in the case's storage, inside a buffer of `fill`: two spare rows, 3 columns in front, at least 2 behind,
    the case's alignment; cols_ld: an exact leading dimension with nothing in front (the edge attributes)"""
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(DEV)
    if cols_ld is not None:
        v = gm.embed(t, 2, 0, cols_ld - t.size(1), fill)
        assert v.stride(0) == cols_ld
        return v
    t = t.to(_dt(case.bf16))
    off, m = am.ALIGN[case.align]
    v = gm.embed(t, 2, 3, am.leading_dim(t.size(1), m), fill, off * t.element_size())
    assert v.stride(0) % 4 == m and v.data_ptr() % 16 == off * t.element_size()
    return v


def out_like(rows, cols, case):
    return place(np.full((rows, cols), LEFT, np.float32), case, CANARY)


def canary_out(rows, cols, case):
    v = out_like(rows, cols, case)
    v.fill_(CANARY)
    return v


def guarded(n):
    """n fp32 outputs with 4 canaries on both sides"""
    buf = torch.full((n + 8,), CANARY, device=DEV)
    return buf, buf[4:4 + n]


def guards_ok(buf):
    return bool((buf[:4] == CANARY).all() and (buf[-4:] == CANARY).all())


def bits(t):
    return t.float().cpu().numpy().view(np.uint32)


def same(t, want):
    return np.array_equal(bits(t), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))


def dev_i32(a):
    """(one spare element behind: an empty index array still has an address, as the entry points require)"""
    return torch.from_numpy(np.concatenate([np.asarray(a, np.int32), np.zeros(1, np.int32)])).to(DEV)[:len(a)]


class Prepared:
    """graph, plans and inputs of a case, on both sides"""

    def __init__(self, case, side, nan_rows=None):
        self.case = case
        self.g = am.build_graph(case, side)
        self.p = am.plans(self.g)
        d = am.family_inputs(case, self.g)
        if nan_rows is not None:
            d = nan_rows(self.g, d)
        self.d = d
        self.fe = {"fused20": 20, "fused2": 2}.get(case.form, 0)
        dead = ~self.g.keep

        def edge_rows(a):          # rows that are no edges of the plan: NaN on the way in
            a = a.copy()
            a[dead] = np.nan
            return a
        self.x, self.da = place(d.x, case, NAN), place(d.da, case, NAN)
        self.phi = place(edge_rows(d.phi), case, NAN) if d.phi is not None else None
        self.ext = place(edge_rows(d.dphi_ext), case, NAN)
        self.add = place(d.add, case, NAN)
        self.ea = self.We = self.be = None
        if d.filter is not None:
            self.ea = place(edge_rows(d.filter.ea), case, NAN, case.lde)
            self.We, self.be = torch.from_numpy(d.filter.We).to(DEV), torch.from_numpy(d.filter.be).to(DEV)
        self.idx = type(self.p)(*(dev_i32(a) for a in self.p))

    def inputs_intact(self):
        return all(gm.outside_intact(v, NAN) for v in (self.x, self.da, self.phi, self.ext, self.add, self.ea) if v is not None)


def fwd_call(s, a, phi_out, eid_none=False, f_e=None, n_dst=None):
    lib, ptr, stream_ptr = _lib()
    c = s.case
    fn = lib.dgnn_sage_aggregate_fwd_bf16 if c.bf16 else lib.dgnn_sage_aggregate_fwd
    ld = lambda v: 0 if v is None else v.stride(0)
    rc = fn(ptr(s.idx.rowptr), ptr(s.idx.src), None if eid_none else ptr(s.idx.eid), s.g.n_dst if n_dst is None else n_dst, ptr(s.x), ld(s.x), c.c_in,
            ptr(s.ea), ld(s.ea), s.fe if f_e is None else f_e, ptr(s.We), ptr(s.be), ptr(s.phi), ld(s.phi), ptr(phi_out), ld(phi_out), ptr(a), ld(a), stream_ptr())
    torch.cuda.synchronize()
    return rc


def bwd_call(s, dx, dphi, dWe, dbe, add=None, n_add=0, ext=None, mask=0, f_e=None, n_src=None, phi="case", entry=None):
    lib, ptr, stream_ptr = _lib()
    c = s.case
    entry = entry or c.entry
    ld = lambda v: 0 if v is None else v.stride(0)
    n_src = s.g.n_src if n_src is None else n_src
    fe = s.fe if f_e is None else f_e
    phi = s.phi if phi == "case" else phi
    head = (ptr(s.idx.t_rowptr), ptr(s.idx.t_dst), ptr(s.idx.t_eid), n_src, ptr(s.idx.rowptr), ptr(s.x), ld(s.x), c.c_in)
    part = None
    if entry in ("bwd", "bwd_add"):
        part = torch.full((int(lib.dgnn_sage_aggregate_bwd_scratch_elems(n_src, c.c_in, fe)),), NAN, device=DEV)
    if entry == "bwd":
        fn = lib.dgnn_sage_aggregate_bwd_bf16 if c.bf16 else lib.dgnn_sage_aggregate_bwd
        rc = fn(*head, ptr(s.ea), ld(s.ea), fe, ptr(s.We), ptr(s.be), ptr(phi), ld(phi), ptr(s.da), ld(s.da), ptr(dx), ld(dx), ptr(dWe), ptr(dbe),
                ptr(dphi), ld(dphi), ptr(part), stream_ptr())
    elif entry == "bwd_add":
        assert not c.bf16
        rc = lib.dgnn_sage_aggregate_bwd_add(*head, ptr(s.ea), ld(s.ea), fe, ptr(s.We), ptr(s.be), ptr(s.da), ld(s.da), ptr(dx), ld(dx), ptr(add), ld(add), n_add,
                                             ptr(dWe), ptr(dbe), ptr(part), stream_ptr())
    else:
        assert entry == "bwd_phi" and (ext is None or dphi is None or ext.stride(0) == dphi.stride(0))
        rc = lib.dgnn_sage_aggregate_bwd_phi_add_masked(*head, ptr(phi), ld(phi), ptr(s.da), ld(s.da), ptr(dx), ld(dx), ptr(add), ld(add), n_add, ptr(dphi),
                                                        ld(dphi) if dphi is not None else ld(ext), ptr(ext), int(c.bf16), mask, stream_ptr())
    torch.cuda.synchronize()
    return rc


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def _cases(*entries):
    cs = [c for c in am.CASES if c.entry in entries]
    return pytest.mark.parametrize("case", cs, ids=[am.case_id(c) for c in cs])


@_cases("fwd")
def test_forward(case):
    """a (and phi_out) equal the model bit for bit; rows of phi_out that are no edges stay as the caller left them; twice the same bits"""
    s = Prepared(case, "dst")
    eid_none = "eid_none" in case.opts
    assert not eid_none or np.array_equal(s.p.eid, np.arange(s.p.eid.size))
    want_a, want_phi = am.forward(s.p.rowptr, s.p.src, None if eid_none else s.p.eid, s.d.x, s.d.filter, s.d.phi, case.bf16)
    runs = []
    for _ in range(2):
        a = out_like(s.g.n_dst, case.c_in, case)
        po = out_like(s.g.ei.shape[1], case.c_in, case) if "phi_out" in case.opts else None
        assert fwd_call(s, a, po, eid_none) == 0
        assert gm.outside_intact(a, CANARY) and (po is None or gm.outside_intact(po, CANARY)) and s.inputs_intact()
        assert same(a, want_a), "a: %d elements differ" % int((bits(a) != want_a.view(np.uint32)).sum())
        if po is not None:
            want = np.where(s.g.keep[:, None], want_phi, np.float32(LEFT))
            assert same(po, want)
        runs.append((a, po))
    assert torch.equal(bits_t(runs[0][0]), bits_t(runs[1][0]))


def bits_t(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def check_backward(case, s, want, n_add, run):
    """run(dx, dphi, dWe, dbe) -> rc, twice; every output against `want` (aggregate_model.Bwd)"""
    o = case.opts
    E_rows = s.g.ei.shape[1]
    fused = s.fe > 0
    first = None
    for _ in range(2):
        dx = None if "no_dx" in o else out_like(s.g.n_src, case.c_in, case)
        dphi = out_like(E_rows, case.c_in, case) if case.form == "given" and "no_dphi" not in o else None
        bufW, dWe = guarded(case.c_in * s.fe) if fused else (None, None)
        bufb, dbe = guarded(case.c_in) if fused else (None, None)
        assert run(dx, dphi, dWe, dbe) == 0
        assert s.inputs_intact()
        if dx is not None:
            assert gm.outside_intact(dx, CANARY)
            assert same(dx, want.dx), "dx: %d elements differ" % int((bits(dx) != want.dx.view(np.uint32)).sum())
        if dphi is not None:
            assert gm.outside_intact(dphi, CANARY)
            assert same(dphi, want.dphi), "dphi: %d elements differ" % int((bits(dphi) != want.dphi.view(np.uint32)).sum())      # (rows that are no edges: as the caller left them)
        if fused:
            assert guards_ok(bufW) and guards_ok(bufb)
            gW, gb = dWe.cpu().numpy().astype(np.float64).reshape(case.c_in, s.fe), dbe.cpu().numpy().astype(np.float64)
            if case.family == "integer":
                assert np.array_equal(gW, want.dWe) and np.array_equal(gb, want.dbe), (np.abs(gW - want.dWe).max(), np.abs(gb - want.dbe).max())
            else:
                B = gm.wgrad_bound(am.wgrad_rho(want))
                for got, ref, mag, what in ((gW, want.dWe, want.magW, "dWe"), (gb, want.dbe, want.magb, "dbe")):
                    err = np.abs(got - ref)
                    ratio = float((err[mag > 0] / (B * mag[mag > 0])).max()) if (mag > 0).any() else 0.0
                    k = am.short_name(am.case_kernel(case, ON))
                    WORST[k] = max(WORST.get(k, 0.0), ratio)
                    print("aggregate %s %s: B %.3g, largest error / (B mag) %.3g; worst of %s so far %.3g" % (am.case_id(case), what, B, ratio, k, WORST[k]))
                    assert np.isfinite(got).all() and (err <= B * mag).all(), (what, ratio)
        now = [None if t is None else bits_t(t).clone() for t in (dx, dphi, dWe, dbe)]
        if first is not None:
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(first, now)), "the second call gave other bits"
        first = now


def dphi_left(s, case):
    """what the caller left in dphi (out_like), as the model takes it"""
    return np.full((s.g.ei.shape[1], case.c_in), LEFT, np.float32)


@_cases("bwd")
def test_backward(case):
    """dgnn_sage_aggregate_bwd / _bf16: dx, dphi, dWe, dbe; without dx and without dphi where the case says so"""
    s = Prepared(case, "src")
    want = am.backward(s.p.t_rowptr, s.p.t_dst, s.p.t_eid, s.p.rowptr, s.d.x, s.d.da, s.d.filter, s.d.phi, bf16=case.bf16, dphi_init=dphi_left(s, case),
                       seq32=case.family != "integer")
    check_backward(case, s, want, 0, lambda dx, dphi, dWe, dbe: bwd_call(s, dx, dphi, dWe, dbe))


@_cases("bwd_add")
def test_backward_with_addend(case):
    """dgnn_sage_aggregate_bwd_add: dx[row] = fl(sum + add[row]) below n_add (0, min(n_src, n_dst) - 1 or n_src), dWe / dbe untouched by it"""
    s = Prepared(case, "src")
    n_add = am.n_add_of(case)
    want = am.backward(s.p.t_rowptr, s.p.t_dst, s.p.t_eid, s.p.rowptr, s.d.x, s.d.da, s.d.filter, add=s.d.add, n_add=n_add, seq32=case.family != "integer")
    check_backward(case, s, want, n_add, lambda dx, dphi, dWe, dbe: bwd_call(s, dx, None, dWe, dbe, add=s.add, n_add=n_add))


@_cases("bwd_phi")
def test_backward_given_phi_with_addend_ext_and_mask(case):
    """dgnn_sage_aggregate_bwd_phi_add_masked: the addend, dphi_ext (one fadd at the store of dphi) and the ReLU mask x > 0 ? dx : +0"""
    s = Prepared(case, "src")
    o = case.opts
    n_add = am.n_add_of(case) if "add" in o else 0
    want = am.backward(s.p.t_rowptr, s.p.t_dst, s.p.t_eid, s.p.rowptr, s.d.x, s.d.da, None, s.d.phi, s.d.add if "add" in o else None, n_add,
                       s.d.dphi_ext if "ext" in o else None, "mask" in o, case.bf16, dphi_left(s, case))
    check_backward(case, s, want, n_add, lambda dx, dphi, dWe, dbe: bwd_call(s, dx, dphi, None, None, add=s.add if "add" in o else None, n_add=n_add,
                                                                             ext=s.ext if "ext" in o else None, mask=int("mask" in o)))


# ---- further edges ------------------------------------------------------------------------------------------------------------------------------
def _c(**kw):
    d = dict(kernel="", entry="bwd", bf16=False, form="fused20", c_in=6, graph="thinned", n_src=257, n_dst=257, family="randn", align="al", lde=20, opts=())
    d.update(kw)
    return am.Case(**d)


# one case per backward form (c, g, mm) and per forward form
LOCAL = [_c(form="fused20", c_in=6), _c(form="fused20", c_in=6, opts=("no_dx",)), _c(form="fused20", c_in=6, align="ldodd"), _c(form="fused20", c_in=7, opts=("no_dx",)),
         _c(form="fused20", c_in=66), _c(form="given", c_in=8), _c(form="given", c_in=8, bf16=True), _c(form="given", c_in=7), _c(form="fused2", c_in=5, lde=2), _c(form="plain", c_in=3),
         _c(form="fused20", c_in=6, graph="ragged", n_src=40, n_dst=400), _c(form="fused20", c_in=6, entry="bwd_add"), _c(form="fused20", c_in=36, bf16=True)]


def _poison(g, d):
    """NaN and Inf in x at source rows without out-edges, in da at destinations without in-edges and in the addend's rows that no case adds"""
    x, da = d.x.copy(), d.da.copy()
    ids = np.nonzero(g.keep)[0]
    s0 = np.nonzero(np.bincount(g.ei[0][ids], minlength=g.n_src) == 0)[0]
    d0 = np.nonzero(np.bincount(g.ei[1][ids], minlength=g.n_dst) == 0)[0]
    assert s0.size >= 1 and d0.size >= 1
    x[s0[0::2]] = np.nan
    x[s0[1::2]] = np.array([np.inf, -np.inf, np.nan] * x.shape[1], np.float32)[:x.shape[1]]
    da[d0] = np.array([np.nan, np.inf] * da.shape[1], np.float32)[:da.shape[1]]
    return d._replace(x=x, da=da)


@pytest.mark.parametrize("case", LOCAL, ids=[am.case_id(c) for c in LOCAL])
def test_non_finite_rows_without_edges_stay_local(case):
    """A source row without out-edges that holds NaN / Inf in x, a destination without in-edges that holds them in da: dWe, dbe, dphi and every
    row's dx are finite and equal the model (which never reads those rows, like autograd over index_select); the forward's `a` is untouched
    too.  Through k_agg_bwd_c, k_agg_bwd_g and k_agg_bwd_mm (with dx, without, with the addend, on the per-edge path)."""
    s = Prepared(case, "src", _poison)
    assert not np.isfinite(s.d.x).all() and not np.isfinite(s.d.da).all()
    n_add = am.n_add_of(case) if case.entry == "bwd_add" else 0
    want = am.backward(s.p.t_rowptr, s.p.t_dst, s.p.t_eid, s.p.rowptr, s.d.x, s.d.da, s.d.filter, s.d.phi, s.d.add if n_add else None, n_add, bf16=case.bf16,
                       dphi_init=dphi_left(s, case))
    assert np.isfinite(want.dx).all() and (want.dWe is None or (np.isfinite(want.dWe).all() and np.isfinite(want.dbe).all()))
    assert want.dphi is None or np.isfinite(want.dphi[s.g.keep]).all()
    check_backward(case, s, want, n_add, lambda dx, dphi, dWe, dbe: bwd_call(s, dx, dphi if case.entry == "bwd" else None, dWe, dbe, add=s.add if n_add else None, n_add=n_add))
    fcase = case._replace(entry="fwd", opts=())
    want_a, _ = am.forward(s.p.rowptr, s.p.src, s.p.eid, s.d.x, s.d.filter, s.d.phi, case.bf16)
    a = out_like(s.g.n_dst, case.c_in, fcase)
    assert fwd_call(s, a, None) == 0 and same(a, want_a) and np.isfinite(want_a).all()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("c_in,align", [(8, "al"), (5, "al"), (130, "ld2")])
def test_mask_dx_edge_values(c_in, align, bf16):
    """x of -0.0, +0.0, NaN, a negative number and -Inf give dx = +0; a positive subnormal, a positive number and +Inf give the sum: x > 0 ? dx : +0
    as IEEE compares, denormals not flushed"""
    case = _c(entry="bwd_phi", form="given", c_in=c_in, align=align, bf16=bf16, graph="tets", n_src=65, n_dst=65, opts=("add", "mask"))
    vals = np.array([-0.0, 0.0, np.nan, 2.0 ** -130, -1.5, 2.5, np.inf, -np.inf, -2.0 ** -130], np.float32)

    def edge_values(g, d):
        x = d.x.copy()
        x.reshape(-1)[:] = vals[np.arange(x.size) % vals.size]
        return d._replace(x=x)
    s = Prepared(case, "src", edge_values)
    da = s.d.da
    n_add = am.n_add_of(case)
    want = am.backward(s.p.t_rowptr, s.p.t_dst, s.p.t_eid, s.p.rowptr, s.d.x, da, None, s.d.phi, s.d.add, n_add, None, True, bf16)
    pos = s.d.x > 0
    assert np.array_equal(want.dx[~pos].view(np.uint32), np.zeros((~pos).sum(), np.uint32)) and (want.dx[pos] != 0).all() and pos[s.d.x == np.float32(2.0 ** -130)].all()
    dx, dphi = out_like(65, c_in, case), out_like(s.g.ei.shape[1], c_in, case)
    assert bwd_call(s, dx, dphi, None, None, add=s.add, n_add=n_add, mask=1) == 0
    assert gm.outside_intact(dx, CANARY) and same(dx, want.dx)
    # mask_dx = 0 is dgnn_sage_aggregate_bwd_phi_add
    want0 = am.backward(s.p.t_rowptr, s.p.t_dst, s.p.t_eid, s.p.rowptr, s.d.x, da, None, s.d.phi, s.d.add, n_add, None, False, bf16)
    dx0 = out_like(65, c_in, case)
    assert bwd_call(s, dx0, dphi, None, None, add=s.add, n_add=n_add, mask=0) == 0 and same(dx0, want0.dx)


def test_no_rows_return_ok_and_write_nothing():
    """n == 0: return code 0, every output keeps its canary; the fused backward zeroes dWe / dbe (they are written, not accumulated)"""
    for bf16 in (False, True):
        for form in ("fused20", "given"):
            case = _c(form=form, bf16=bf16, graph="tets", n_src=17, n_dst=17)
            s = Prepared(case, "src")
            a, dx, dphi = canary_out(17, 6, case), canary_out(17, 6, case), canary_out(68, 6, case) if form == "given" else None
            bufW, dWe = guarded(6 * s.fe) if s.fe else (None, None)
            bufb, dbe = guarded(6) if s.fe else (None, None)
            assert fwd_call(s, a, None, n_dst=0) == 0 and bool((a._base == CANARY).all())
            assert bwd_call(s, dx, dphi, dWe, dbe, n_src=0) == 0 and bool((dx._base == CANARY).all()) and (dphi is None or bool((dphi._base == CANARY).all()))
            if s.fe:
                assert guards_ok(bufW) and guards_ok(bufb) and bool((dWe == 0).all()) and bool((dbe == 0).all())


def test_refusals_launch_nothing():
    """f_e outside {2, 20}, an addend without dx, dphi_ext without a given phi, n_add > n_src (and < 0): the documented error code, and every
    output buffer keeps its canary in every element"""
    case = _c(graph="tets", n_src=17, n_dst=17)
    s = Prepared(case, "src")
    sg = Prepared(_c(form="given", entry="bwd_phi", graph="tets", n_src=17, n_dst=17), "src")
    outs = []

    def fresh(s_, rows):
        v = canary_out(rows, 6, s_.case)
        outs.append(v)
        return v

    def W():
        buf, v = guarded(6 * 20)
        outs.append(buf)
        return v
    for fe in (3, 19, 21):
        assert fwd_call(s, fresh(s, 17), None, f_e=fe) == E_UNSUPPORTED
        assert bwd_call(s, fresh(s, 17), None, W(), W(), f_e=fe) == E_UNSUPPORTED
    assert bwd_call(s, None, None, W(), W(), add=s.add, n_add=3, entry="bwd_add") == E_UNSUPPORTED                     # an addend without dx
    assert bwd_call(sg, None, fresh(sg, 68), None, None, add=sg.add, n_add=3) == E_UNSUPPORTED
    assert bwd_call(sg, fresh(sg, 17), fresh(sg, 68), None, None, ext=sg.ext, phi=None) == E_UNSUPPORTED              # dphi_ext without a given phi
    assert bwd_call(sg, fresh(sg, 17), None, None, None, ext=sg.ext) == E_UNSUPPORTED                                # ... and without dphi_out
    assert bwd_call(sg, None, fresh(sg, 68), None, None, mask=1) == E_UNSUPPORTED                                    # the masked store without dx
    for n_add in (18, -1):
        assert bwd_call(s, fresh(s, 17), None, W(), W(), add=s.add, n_add=n_add, entry="bwd_add") == E_INVALID
        assert bwd_call(sg, fresh(sg, 17), fresh(sg, 68), None, None, add=sg.add, n_add=n_add) == E_INVALID
    for v in outs:
        assert bool(((v if v._base is None else v._base) == CANARY).all())
