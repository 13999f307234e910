"""tests/aggregate_model.py checked on the CPU: fmaf32 against exact rational arithmetic, forward / backward against the oracle's propagate_mean
(bit for bit), against an fp64 autograd evaluation (inside the rounding bound; equal in the integer family), the case table against the
restated dispatch (every instantiation reached, every row names the kernel it reaches) and the sizes against the pass thresholds."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import aggregate_model as am

F32 = np.float32
U = 2.0 ** -24


def _round_f32(q):
    """a Fraction rounded to the nearest fp32, ties to even (normal and subnormal range)"""
    if q == 0:
        return F32(0.0)
    s, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)
    ulp = Fraction(2) ** (e - 23)
    n = q / ulp
    f = n.numerator // n.denominator
    rem = n - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return F32(s * float(f * ulp))


def _fma_exact(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_fmaf32_constructed_ties():
    """fmaf(1 + 2^-20, 0.5 (1 - 2^-20), 2^23 + 1): the exact sum 2^23 + 1.5 - 2^-41 rounds to 2^23 + 1.5 in fp64, an fp32 tie that float32()
    sends to the even 2^23 + 2; one rounding gives 2^23 + 1.  The mirror images: negated, and at the next such tie, 2^23 + 3.5; an exact tie keeps
    the even rule.  (Remainders on the other side of a tie are among the random near-ties of the next test.)"""
    a, b = F32(1 + 2.0 ** -20), F32(0.5 * (1 - 2.0 ** -20))
    c = F32(2.0 ** 23 + 1)
    assert float(np.float32(np.float64(a) * np.float64(b) + np.float64(c))) == 2.0 ** 23 + 2          # the naive form is wrong
    assert float(am.fmaf32(a, b, c)) == 2.0 ** 23 + 1
    assert float(am.fmaf32(-a, b, -c)) == -(2.0 ** 23 + 1)
    c2 = F32(2.0 ** 23 + 3)                                                                           # the next tie whose odd neighbour is below
    assert float(am.fmaf32(a, b, c2)) == 2.0 ** 23 + 3 and float(np.float32(np.float64(a) * np.float64(b) + np.float64(c2))) == 2.0 ** 23 + 4
    assert float(am.fmaf32(a, -b, -c2)) == -(2.0 ** 23 + 3)
    assert float(am.fmaf32(F32(1), F32(0.5), F32(2.0 ** 23 + 1))) == 2.0 ** 23 + 2                     # an exact tie keeps the even rule
    assert float(am.fmaf32(F32(1), F32(0.5), F32(2.0 ** 23))) == 2.0 ** 23
    for t in [(a, b, c), (-a, b, -c), (a, b, c2), (a, -b, -c), (F32(1), F32(0.5), F32(2.0 ** 23 + 1))]:
        assert am.fmaf32(*t) == _fma_exact(*t)


def test_fmaf32_equals_exact_rational_arithmetic():
    """random triples: plain, with cancellation (c about -a b), with c far larger and far smaller than a b, near-tie sums built like the
    constructed one, and results in the subnormal range"""
    r = np.random.default_rng(5)
    n = 400
    a = r.standard_normal(n).astype(F32)
    b = r.standard_normal(n).astype(F32)
    sets = [(a, b, r.standard_normal(n).astype(F32)), (a, b, (-(a * b) * F32(1 + 2.0 ** -12)).astype(F32)),
            (a, b, (r.standard_normal(n) * 2.0 ** 24).astype(F32)), (a, b, (r.standard_normal(n) * 2.0 ** -30).astype(F32)),
            ((1 + r.integers(1, 2 ** 23, n) * 2.0 ** -23).astype(F32), (0.5 * (1 + r.integers(-2 ** 22, 2 ** 22, n) * 2.0 ** -23)).astype(F32),
             (2.0 ** 23 + r.integers(0, 2 ** 22, n)).astype(F32)),
            ((a * F32(2.0 ** -70)).astype(F32), (b * F32(2.0 ** -62)).astype(F32), (r.standard_normal(n) * 2.0 ** -140).astype(F32))]
    for aa, bb, cc in sets:
        got = am.fmaf32(aa, bb, cc)
        want = np.array([_fma_exact(x, y, z) for x, y, z in zip(aa, bb, cc)], F32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_bf16_round_is_torch():
    r = np.random.default_rng(6)
    v = np.concatenate([(r.standard_normal(4000) * np.exp2(r.integers(-20, 20, 4000))).astype(F32), np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 0.0, -0.0], F32)])
    assert np.array_equal(am.bf16_round(v), torch.from_numpy(v).to(torch.bfloat16).float().numpy())


def _case(**kw):
    d = dict(kernel="", entry="bwd", bf16=False, form="fused20", c_in=5, graph="ragged", n_src=40, n_dst=33, family="randn", align="al", lde=20, opts=())
    d.update(kw)
    return am.Case(**d)


@pytest.mark.parametrize("graph,n_src,n_dst", [("ragged", 40, 33), ("thinned", 129, 129), ("chunk64", 23, 23)])
def test_forward_given_and_plain_are_propagate_mean(graph, n_src, n_dst):
    """the model's forward with a given phi and without a filter equals oracle.pyg_semantics.propagate_mean in fp32 bit for bit (edges in list
    order per destination = plan order of the stable sort), with and without edge ids"""
    from oracle.pyg_semantics import propagate_mean
    case = _case(entry="fwd", form="given", graph=graph, n_src=n_src, n_dst=n_dst)
    g = am.build_graph(case, "dst")
    p = am.plans(g)
    d = am.family_inputs(case, g)
    ids = np.nonzero(g.keep)[0]
    ei = torch.from_numpy(g.ei[:, ids])
    for phi in (d.phi, None):
        want = propagate_mean(torch.from_numpy(d.x), g.n_dst, ei, None if phi is None else torch.from_numpy(phi[ids])).numpy()
        a, _ = am.forward(p.rowptr, p.src, p.eid, d.x, phi=phi)
        assert np.array_equal(a.view(np.uint32), want.view(np.uint32))
    gg = am.grouped_by_dst(g)
    pg = am.plans(gg)
    assert np.array_equal(pg.eid, np.arange(ids.size))
    o = ids[np.argsort(g.ei[1][ids], kind="stable")]
    a2, _ = am.forward(pg.rowptr, pg.src, None, d.x, phi=d.phi[o])
    a1, _ = am.forward(p.rowptr, p.src, p.eid, d.x, phi=d.phi)
    assert np.array_equal(a1, a2)


def _autograd64(g, d, n_add, mask_dx, add, ext):
    """fp64 autograd over index_select / index_add_ -> a, phi, dx, dphi (plan rows), dWe, dbe and the magnitudes |.| of a and dx"""
    ids = np.nonzero(g.keep)[0]
    s, t = torch.from_numpy(g.ei[0][ids]), torch.from_numpy(g.ei[1][ids])
    x = torch.from_numpy(d.x).double().requires_grad_()
    da = torch.from_numpy(d.da).double()
    deg = torch.bincount(t, minlength=g.n_dst).clamp_min(1).double()[:, None]
    We = be = None
    if d.filter is not None:
        ea, We, be = (torch.from_numpy(v).double() for v in d.filter)
        We.requires_grad_(), be.requires_grad_()
        phi = ea[ids] @ We.t() + be
        phimag = ea[ids].abs() @ We.abs().t().detach() + be.abs().detach()
    elif d.phi is not None:
        phi = torch.from_numpy(d.phi[ids]).double().requires_grad_()
        phimag = phi.abs().detach()
    else:
        phi, phimag = None, torch.ones(ids.size, x.size(1), dtype=torch.float64)
    m = x[s] if phi is None else x[s] * phi
    a = torch.zeros(g.n_dst, x.size(1), dtype=torch.float64).index_add_(0, t, m) / deg
    amag = torch.zeros_like(a).index_add_(0, t, (x[s].abs() * phimag).detach()) / deg
    (a * da).sum().backward()
    dx = x.grad.clone()
    dxmag = torch.zeros_like(dx).index_add_(0, s, (da[t] / deg[t]).abs() * phimag)
    if add is not None:
        dx[:n_add] += torch.from_numpy(add[:n_add]).double()
        dxmag[:n_add] += torch.from_numpy(add[:n_add]).double().abs()
    if mask_dx:
        dx = torch.where(x.detach() > 0, dx, torch.zeros_like(dx))
    dphi = None
    if d.filter is None and phi is not None:
        dphi = phi.grad + (0 if ext is None else torch.from_numpy(ext[ids]).double())
    return dict(a=a.detach().numpy(), amag=amag.numpy(), phi=None if phi is None else phi.detach().numpy(), dx=dx.numpy(), dxmag=dxmag.numpy(),
                dphi=None if dphi is None else dphi.numpy(), dWe=None if We is None else We.grad.numpy(), dbe=None if be is None else be.grad.numpy(), ids=ids)


FORMS = [("fused20", ()), ("fused2", ()), ("given", ("add", "ext", "mask")), ("given", ()), ("plain", ()), ("fused20", ("add",))]


@pytest.mark.parametrize("form,opts", FORMS)
@pytest.mark.parametrize("family", ["randn", "wide", "integer"])
def test_model_against_fp64_autograd(form, opts, family):
    """forward and backward of every form: each element within (terms + attributes + 4) 2^-24 of its magnitude sum around the fp64 autograd value
    (one rounding per product, per partial sum, per fmaf of the filter chain, the division, the addend); in the integer family dx, dphi, dWe and
    dbe equal fp64 exactly and `a` is the fp64 quotient rounded once (an exact numerator: double rounding of a quotient is innocuous at 53 >=
    2 * 24 + 2 bits)"""
    case = _case(form=form, family=family, opts=opts, lde={"fused2": 2}.get(form, 20))
    g = am.build_graph(case, "src")
    p = am.plans(g)
    d = am.family_inputs(case, g)
    n_add = am.n_add_of(case) if "add" in opts else 0
    add = d.add if "add" in opts else None
    ext = d.dphi_ext if "ext" in opts else None
    ref = _autograd64(g, d, n_add, "mask" in opts, add, ext)
    fe = 0 if d.filter is None else d.filter.We.shape[1]
    a, phi = am.forward(p.rowptr, p.src, p.eid, d.x, d.filter, d.phi)
    b = am.backward(p.t_rowptr, p.t_dst, p.t_eid, p.rowptr, d.x, d.da, d.filter, d.phi, add, n_add, ext, "mask" in opts)
    maxdeg = 131
    bound = (maxdeg + fe + 4) * U
    exact = family == "integer"
    if exact:
        assert np.array_equal(a, ref["a"].astype(F32)) and np.array_equal(b.dx.astype(np.float64), ref["dx"])
    else:
        assert (np.abs(a - ref["a"]) <= bound * ref["amag"]).all() and (np.abs(b.dx - ref["dx"]) <= bound * ref["dxmag"]).all()
        assert np.abs(a - ref["a"]).max() > 0                  # not fp64 in disguise
    if phi is not None:
        err = np.abs(phi[ref["ids"]] - ref["phi"])
        assert (err == 0).all() if exact else (err <= (fe + 1) * U * (np.abs(d.filter.ea[ref["ids"]]) @ np.abs(d.filter.We).T + np.abs(d.filter.be))).all()
    if b.dphi is not None:
        got = b.dphi[ref["ids"]]
        assert np.isnan(b.dphi[~g.keep]).all() and not np.isnan(got).any()
        if exact:
            assert np.array_equal(got.astype(np.float64), ref["dphi"])
        else:
            assert (np.abs(got - ref["dphi"]) <= 3 * U * (np.abs(ref["dphi"]) + (0 if ext is None else np.abs(ext[ref["ids"]])))).all()
    if fe:
        # the model's fp64 sums are sums of the fp32 dphi: they differ from autograd's by dphi's own rounding (2 roundings per term)
        for got, seq, mag, want in ((b.dWe, b.seqW, b.magW, ref["dWe"]), (b.dbe, b.seqb, b.magb, ref["dbe"])):
            if exact:
                assert np.array_equal(got, want) and np.array_equal(seq.astype(np.float64), want)
            else:
                assert (np.abs(got - want) <= 3 * U * mag).all()
                assert (np.abs(seq - got) <= (int(g.keep.sum()) + 1) * U * mag).all()
        assert exact or am.wgrad_rho(b) > 0
        assert not exact or am.wgrad_rho(b) == 0


def test_bf16_storage_rounds_inputs_and_outputs_only():
    """bf16 storage = the fp32 model on the inputs as stored, outputs rounded once; `a` from the unrounded phi"""
    case = _case(bf16=True, form="fused20", c_in=6)
    g = am.build_graph(case, "src")
    p = am.plans(g)
    d = am.family_inputs(case, g)
    assert np.array_equal(am.bf16_round(d.x), d.x) and not np.array_equal(am.bf16_round(d.filter.ea), d.filter.ea)
    a32, phi32 = am.forward(p.rowptr, p.src, p.eid, d.x, d.filter)
    a16, phi16 = am.forward(p.rowptr, p.src, p.eid, d.x, d.filter, bf16=True)
    assert np.array_equal(a16, am.bf16_round(a32)) and np.array_equal(phi16, am.bf16_round(phi32)) and not np.array_equal(phi16, phi32)
    b32 = am.backward(p.t_rowptr, p.t_dst, p.t_eid, p.rowptr, d.x, d.da, d.filter)
    b16 = am.backward(p.t_rowptr, p.t_dst, p.t_eid, p.rowptr, d.x, d.da, d.filter, bf16=True)
    assert np.array_equal(b16.dx, am.bf16_round(b32.dx)) and np.array_equal(b16.dWe, b32.dWe)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------
def test_every_row_names_the_kernel_it_reaches_and_every_instantiation_is_reached():
    reached = set()
    for c in am.CASES:
        full = am.case_kernel(c)
        assert am.short_name(full) == c.kernel, (am.case_id(c), full)
        reached.add(full)
    want = am.all_instantiations()
    assert reached <= want, reached - want
    assert want <= reached, sorted(want - reached)
    ids = [am.case_id(c) for c in am.CASES]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    assert len(am.CASES) < 400


def test_switches_move_the_cases_to_the_other_kernels():
    """DGNN_AGG_GROUPED=0: no lane-group kernel; DGNN_AGG_MFMA=0: no matrix-core kernel; DGNN_AGG_BWD_NODX=0 (with MFMA off): no no-dx form"""
    on = {s: True for s in am.SWITCHES}
    for off, gone in ((("DGNN_AGG_GROUPED",), ("_g<",)), (("DGNN_AGG_MFMA",), ("_m<", "_mm<")), (("DGNN_AGG_BWD_NODX", "DGNN_AGG_MFMA"), (",-,->", "_m<", "_mm<"))):
        sw = dict(on, **{s: False for s in off})
        names = {am.case_kernel(c, sw) for c in am.CASES}
        assert not [n for n in names if any(t in n for t in gone)]
        assert names <= am.all_instantiations()
    assert am.env_switches({"DGNN_AGG_MFMA": "0"}) == dict(on, DGNN_AGG_MFMA=False)


def test_widths_and_forms_of_the_table():
    w = lambda entry, form: {c.c_in for c in am.CASES if c.entry.startswith(entry) and c.form == form}
    assert w("fwd", "given") >= {4, 8, 28, 32, 36, 60, 64, 68, 124, 128, 132, 129, 1, 200} and w("bwd", "given") >= {4, 8, 28, 32, 36, 60, 64, 68, 124, 128, 132, 129, 1, 200}
    assert w("fwd", "fused20") >= {2, 6, 30, 32, 34, 36, 60, 64, 66, 65, 128, 130, 129, 1} and w("bwd", "fused20") >= {2, 6, 30, 32, 34, 36, 60, 64, 66, 65, 128, 130, 129, 1}
    assert w("fwd", "fused2") >= {1, 48, 130} and w("bwd", "fused2") >= {1, 48, 130} and w("fwd", "plain") >= {1, 28, 130} and w("bwd", "plain") >= {1, 28, 130}
    for entry in ("fwd", "bwd"):
        assert {c.n_src for c in am.CASES if c.entry == entry} >= set(am.SIZES_SMALL) | set(am.SIZES_LARGE)
        assert {c.align for c in am.CASES if c.entry == entry} == set(am.ALIGN) and {c.lde for c in am.CASES if c.entry == entry and c.form == "fused20"} == {20, 23}
    assert any(c.n_src > c.n_dst for c in am.CASES) and any(c.n_src < c.n_dst for c in am.CASES)
    for c in am.CASES:
        o = am.case_operands(c)["x"]
        assert o[1] >= c.c_in + 5 and o[1] % 4 == am.ALIGN[c.align][1]


def test_thresholds():
    """chunk_rows, the pass counts and the slab counts at the table's sizes, from the constants of aggregate.hip and common.h"""
    assert [am.chunk_rows(n) for n in (1, 16384, 16385, 32768, 32769, 49152, 49153, 131093)] == [4, 4, 8, 8, 12, 12, 16, 16]
    assert [am.passes("k_agg_fwd", n) for n in (8192, 8193, 16385)] == [1, 2, 3]
    for k in ("k_agg_bwd_c", "k_agg_bwd_mm", "k_agg_fwd_m4"):
        assert [am.passes(k, n) for n in (49153, 65536, 65541, 131072, 131093)] == [1, 1, 2, 2, 3], k
    for k in ("k_agg_fwd_m2", "k_agg_fwd_g", "k_agg_bwd_g"):
        assert [am.passes(k, n) for n in (65541, 131072, 131093)] == [1, 1, 2], k
    assert [am.bwd_blocks(n, am.chunk_rows(n)) for n in (16368, 16369, 16384, 16385, 65472, 65473, 65541)] == [1023, 1024, 1024, 513, 1023, 1024, 1024]
    big = {k: max(c.n_src for c in am.CASES if c.kernel.startswith(k)) for k in ("k_agg_fwd<", "k_agg_fwd_g", "k_agg_fwd_m<2", "k_agg_fwd_m<4", "k_agg_bwd_g", "k_agg_bwd_c", "k_agg_bwd_mm")}
    assert am.passes("k_agg_fwd", big["k_agg_fwd<"]) >= 2 and am.passes("k_agg_fwd_g", big["k_agg_fwd_g"]) == 2 and am.passes("k_agg_fwd_m2", big["k_agg_fwd_m<2"]) == 2
    assert am.passes("k_agg_fwd_m4", big["k_agg_fwd_m<4"]) == 3 and am.passes("k_agg_bwd_g", big["k_agg_bwd_g"]) == 2
    assert am.passes("k_agg_bwd_c", big["k_agg_bwd_c"]) == 3 and am.passes("k_agg_bwd_mm", big["k_agg_bwd_mm"]) == 3
    # every chunk size of the chunked kernels, and the capped 1024 slabs with 4-row and with 16-row chunks
    for k in ("k_agg_fwd_g", "k_agg_bwd_g", "k_agg_bwd_c"):
        assert {am.chunk_rows(c.n_src if c.entry != "fwd" else c.n_dst) for c in am.CASES if c.kernel.startswith(k)} == {4, 8, 12, 16}, k
    fused = [c for c in am.CASES if c.entry in ("bwd", "bwd_add") and c.form == "fused20" and c.kernel.startswith("k_agg_bwd_c")]
    assert {(am.chunk_rows(c.n_src), am.bwd_blocks(c.n_src, am.chunk_rows(c.n_src))) for c in fused} >= {(4, 1024), (8, 513), (16, 1024)}


@pytest.mark.parametrize("n", [23, 49153])
def test_chunk64_builds_the_chunk_totals(n):
    """under chunk_rows(n) the first five chunks of the walked plan hold 63, 64, 65, 64 and 65 edges with the documented row degrees, later chunks
    4 per row (64 per 16-row chunk), the array ends (0, 5, 0); on the side that is walked: in-degrees for 'dst', out-degrees for 'src'"""
    rw = am.chunk_rows(n)
    assert rw == (4 if n == 23 else 16)
    for side in ("dst", "src"):
        g = am.chunk64(n, side)
        p = am.plans(g)
        rp = (p.rowptr if side == "dst" else p.t_rowptr).astype(np.int64)
        deg = np.diff(rp)
        tot = [int(rp[min((k + 1) * rw, n)] - rp[k * rw]) for k in range(-(-n // rw))]
        assert tot[:5] == [63, 64, 65, 64, 65]
        assert set(tot[5:-2]) <= {64 if rw == 16 else 16} and list(deg[-3:]) == [0, 5, 0]
        q = 64 // rw
        assert list(deg[:rw]) == [q] * (rw - 1) + [q - 1] and list(deg[2 * rw:3 * rw]) == [q] * (rw - 1) + [q + 1]
        assert list(deg[3 * rw:4 * rw]) == [0] * (rw - 1) + [64] and list(deg[4 * rw:5 * rw]) == [65] + [0] * (rw - 1)


def test_graph_builders():
    for n in am.SIZES_SMALL + (257,):
        g = am.tets(n)
        assert (np.bincount(g.ei[0], minlength=n) == 4).all() and (np.bincount(g.ei[1], minlength=n) == 4).all()
        assert np.array_equal(g.ei[0], np.repeat(np.arange(n), 4))
    g = am.thinned(257)
    assert not g.keep.all() and am.plans(g).t_eid.size == g.keep.sum()
    g = am.ragged(40, 33)
    p = am.plans(g)
    od = np.diff(p.t_rowptr)
    assert {64, 65, 130} <= set(od) and 130 in set(np.diff(p.rowptr)) and od[0] == 0 and od[-1] == 0
    assert am.plans(am.empty(9, 7)).rowptr.tolist() == [0] * 8


def test_the_largest_case_evaluates_in_seconds():
    import time
    c = max((c for c in am.CASES if c.form == "fused20" and c.entry == "bwd"), key=lambda c: (c.n_src, c.c_in))
    assert c.n_src == 131093
    t = time.time()
    g = am.build_graph(c, "src")
    p = am.plans(g)
    d = am.family_inputs(c, g)
    b = am.backward(p.t_rowptr, p.t_dst, p.t_eid, p.rowptr, d.x, d.da, d.filter, seq32=False)
    assert np.array_equal(b.dWe, np.round(b.dWe)) and np.abs(b.magW).max() < 2 ** 24
    assert time.time() - t < 20
