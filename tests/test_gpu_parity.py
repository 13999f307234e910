"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the committed golden
vectors.  Bar: bit-exact for integer/index work; fp32 logits within 1e-4 abs (the
reference differs from its own fp64 evaluation by 4e-6; the downstream graph cut rounds logit*10)."""
import os

import numpy as np
import pytest
import torch

from dgnn_amd.config import Config, reconbench_pretrained
from helpers import f3_data, gold, kf96_state_dict, oracle_static

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL_LOGIT = 1e-4


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def hip_static(train=False, convs=(64, 128, 128, 128), sd=None):
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import SurfaceNet
    net = SurfaceNet(reconbench_pretrained(device=DEV, convs=convs))
    net.load_state_dict(kf96_state_dict() if sd is None else sd)
    net = net.to(DEV)
    return net.train() if train else net.eval()


# ---- plan: bit-exact index work -------------------------------------------------------------------
@pytest.mark.parametrize("case", ["regular", "ragged", "empty_rows", "star", "empty", "grouped", "grouped_but_one"])
def test_plan_matches_stable_sort(case):
    from dgnn_amd import ops
    rng = np.random.default_rng(0)
    if case == "regular":
        from dgnn_amd.synthetic import delaunay_tet_graph
        adj, _, _ = delaunay_tet_graph(3000, seed=2)
        ei = adj.T.astype(np.int64)
        n_src = n_dst = adj.shape[0] // 4
    elif case == "ragged":
        n_src, n_dst, E = 5000, 3000, 40000
        ei = np.stack([rng.integers(0, n_src, E), rng.integers(0, n_dst, E)])
    elif case in ("grouped", "grouped_but_one"):
        # edge list already grouped by destination (sampled blocks, partition-local lists): the identity fast path,
        # with empty rows at the start, in the middle and at the end; one inversion must send it to the generic kernels
        n_src, n_dst, E = 3000, 2000, 9000
        dst = np.sort(rng.integers(5, n_dst - 7, E))
        dst[(dst > 700) & (dst < 760)] = 760
        if case == "grouped_but_one":
            dst[4000], dst[4001] = dst[4001] + 1, dst[4000]
        ei = np.stack([rng.integers(0, n_src, E), dst])
    elif case == "empty_rows":
        n_src, n_dst, E = 100, 1000, 300
        ei = np.stack([rng.integers(0, n_src, E), rng.integers(0, n_dst, E)])
    elif case == "star":  # one destination with a very long segment + some medium ones
        n_src, n_dst = 4000, 50
        dst = np.concatenate([np.zeros(3000, np.int64), rng.integers(1, 5, 200), rng.integers(5, 50, 500)])
        ei = np.stack([rng.integers(0, n_src, dst.shape[0]), rng.permutation(dst)])
    else:
        n_src, n_dst = 7, 5
        ei = np.zeros((2, 0), np.int64)
    _check_plan(ops, ei, n_src, n_dst)


def _check_plan(ops, ei, n_src, n_dst):
    # both memory layouts the reference produces: a contiguous [2,E] tensor and the transposed view of the [E,2] array
    # (torch.transpose(adjacencies,1,0), processing/data.py:437-438); the builder reads either in place
    views = [torch.from_numpy(np.ascontiguousarray(ei)).to(DEV), torch.from_numpy(np.ascontiguousarray(ei.T)).to(DEV).t()]
    assert not views[1].is_contiguous() or ei.shape[1] <= 1
    for t in views:
        for by, n_key in ((1, n_dst), (0, n_src)):
            key, oth = ei[by], ei[1 - by]
            order = np.argsort(key, kind="stable")
            ref_rowptr = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n_key))])
            # the hint only chooses which verified fast path is attempted; a wrong hint must still give the stable sort
            for hint in (ops.PLAN_HINT_AUTO, ops.PLAN_HINT_GROUPED, ops.PLAN_HINT_REFERENCE):
                rowptr, other, eid = ops.plan_build(t, n_key, by, hint)
                assert np.array_equal(rowptr.cpu().numpy(), ref_rowptr), (by, hint)
                assert np.array_equal(eid.cpu().numpy(), order), (by, hint)
                assert np.array_equal(other.cpu().numpy(), oth[order]), (by, hint)


@pytest.mark.parametrize("case", ["delaunay", "duplicates_selfloops", "one_way", "wrong_group", "out_of_pattern_src", "perm_rows"])
def test_plan_regular_fast_path_and_its_fallback(case):
    """E == 4N graphs: the reference layout takes the verified single-pass builder; every near miss (asymmetric relation,
    rows not grouped by source, ...) must be caught on the device and rebuilt by the generic kernels -- the result is
    always the stable sort."""
    from dgnn_amd import ops
    from dgnn_amd.synthetic import delaunay_tet_graph
    rng = np.random.default_rng(3)
    adj, _, _ = delaunay_tet_graph(2500, seed=4)
    n = adj.shape[0] // 4
    ei = adj.T.astype(np.int64).copy()
    if case == "duplicates_selfloops":
        # symmetric multigraph in the reference layout: double links a<->b (two slots each way) and self loops
        n = 64
        nb = np.empty((n, 4), np.int64)
        # even cells: a double link to the odd partner + a ring over the even cells; odd cells: the double link + 2 self loops
        for a in range(0, n, 2):
            nb[a] = [a + 1, a + 1, (a + 2) % n, (a - 2) % n]
            nb[a + 1] = [a, a, a + 1, a + 1]
        ei = np.stack([np.repeat(np.arange(n), 4), nb.reshape(-1)])
    elif case == "one_way":
        k = 4 * 17 + 2
        ei[1, k] = (ei[1, k] + 7) % n                     # one link no longer has its reverse
    elif case == "wrong_group":
        ei[0, [5, 9]] = ei[0, [9, 5]]                      # sources 1 and 2 have 3 and 5 rows: still E == 4N
    elif case == "out_of_pattern_src":
        ei = ei[:, rng.permutation(ei.shape[1])]           # same graph, rows shuffled
    elif case == "perm_rows":
        p = (np.arange(n)[:, None] * 4 + np.array([2, 0, 3, 1])[None]).reshape(-1)
        ei = ei[:, p]                                      # still grouped by source, slots permuted: fast path holds
    _check_plan(ops, ei, n, n)


# ---- aggregate: given phi is bit-exact against the oracle's propagate ------------------------------
@pytest.mark.parametrize("c_in", [28, 64, 128, 200])
def test_aggregate_phi_given_bit_exact(c_in):
    from dgnn_amd import ops
    from oracle.pyg_semantics import propagate_mean
    g = torch.Generator().manual_seed(c_in)
    n_src, n_dst, E = 700, 500, 2600
    ei = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst + 40, (E,), generator=g).clamp_max(n_dst - 1)])
    x = torch.randn(n_src, c_in, generator=g)
    phi = torch.randn(E, c_in, generator=g)
    ref = propagate_mean(x, n_dst, ei, phi)
    rowptr, src, eid = ops.plan_build(ei.to(DEV), n_dst, 1)
    a = ops.aggregate_fwd(rowptr, src, eid, n_dst, x.to(DEV), phi=phi.to(DEV))
    assert torch.equal(a.cpu(), ref)
    ref_plain = propagate_mean(x, n_dst, ei, None)
    a = ops.aggregate_fwd(rowptr, src, eid, n_dst, x.to(DEV))
    assert torch.equal(a.cpu(), ref_plain)


@pytest.mark.parametrize("c_in,f_e", [(28, 20), (64, 20), (128, 20), (48, 2)])
def test_aggregate_fused_filter(c_in, f_e):
    from dgnn_amd import ops
    from oracle.pyg_semantics import propagate_mean
    g = torch.Generator().manual_seed(7)
    n_src, n_dst, E = 900, 600, 3000
    ei = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    x = torch.randn(n_src, c_in + 1, generator=g)[:, 1:]  # unaligned view, row stride c_in+1
    ea = torch.randn(E, f_e, generator=g)
    We, be = torch.randn(c_in, f_e, generator=g) * 0.3, torch.randn(c_in, generator=g)
    phi64 = ea.double() @ We.double().t() + be.double()
    ref = propagate_mean(x.double(), n_dst, ei, phi64)
    rowptr, src, eid = ops.plan_build(ei.to(DEV), n_dst, 1)
    xd = torch.randn(1).to(DEV)  # noqa: F841 (touch the device)
    x_dev = torch.empty(n_src, c_in + 1, device=DEV)
    x_dev[:, 1:] = x.to(DEV)
    a, phi = ops.aggregate_fwd(rowptr, src, eid, n_dst, x_dev[:, 1:], ea.to(DEV), We.to(DEV), be.to(DEV), want_phi=True)
    assert rel_err(a, ref) < 2e-6
    assert rel_err(phi, phi64) < 2e-6


@pytest.mark.parametrize("c_in,n_src,n_dst", [(28, 5000, 1777), (64, 900, 600), (32, 70, 70), (128, 800, 500), (48, 300, 203), (20, 64, 5), (64, 9, 1), (28, 40, 17)])
def test_lane_group_fused_filter_forward_gives_the_bits_of_the_lane_per_channel_kernel(c_in, n_src, n_dst):
    """k_agg_fwd_m (round 6: the filter product on the fp32 matrix cores, 4 edge slots per destination row; DGNN_AGG_MFMA=0: k_agg_fwd on both
    sides) against k_agg_fwd (taken when the row stride of x is no multiple
    of 4): the aggregate bit for bit; regular, ragged (a row of more than 4 in-edges sends its step to the per-edge path) and thinned in-degrees"""
    from dgnn_amd import ops
    if os.environ.get("DGNN_AGG_GROUPED") == "0":
        pytest.skip("compares the two default kernels")
    g = torch.Generator().manual_seed(c_in + n_src)
    E = 4 * n_dst
    x = torch.randn(n_src, c_in, generator=g).to(DEV)
    xw = torch.zeros(n_src, c_in + 1, device=DEV)
    xw[:, :c_in] = x
    ea = torch.randn(E, 20, generator=g).to(DEV)
    We, be = (torch.randn(c_in, 20, generator=g) * 0.3).to(DEV), torch.randn(c_in, generator=g).to(DEV)
    ei = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.arange(n_dst).repeat_interleave(4)])
    ei2 = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    ei2[1, : E // 4] = ei2[1, : E // 4] % 11
    ei3 = ei[:, torch.rand(E, generator=g) < 0.7]        # in-degrees 0 .. 4: the matrix-core form's partly filled edge slots (k_agg_fwd_m, round 6)
    for edges in (ei, ei2, ei3):
        rp, src, eid = ops.plan_build(edges.to(DEV), n_dst, 1)
        a_g = ops.aggregate_fwd(rp, src, eid, n_dst, x, ea, We, be)
        a_c = ops.aggregate_fwd(rp, src, eid, n_dst, xw[:, :c_in], ea, We, be)
        assert torch.equal(a_g, a_c)


# ---- dense kernels ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M,k1,k2,n_out", [(1000, 28, 28, 64), (777, 64, 64, 128), (2048, 128, 128, 128), (300, 128, 0, 2),
                                          (130, 37, 5, 70), (1, 128, 0, 64)])
def test_linear_fwd(M, k1, k2, n_out):
    from dgnn_amd import ops
    g = torch.Generator().manual_seed(M)
    A1, W1 = torch.randn(M, k1, generator=g), torch.randn(n_out, k1, generator=g)
    b = torch.randn(n_out, generator=g)
    sc, sh = torch.rand(n_out, generator=g) + 0.5, torch.randn(n_out, generator=g)
    ref = A1.double() @ W1.double().t() + b.double()
    args = dict(A1=A1.to(DEV), W1=W1.to(DEV), bias=b.to(DEV))
    if k2:
        A2, W2 = torch.randn(M, k2, generator=g), torch.randn(n_out, k2, generator=g)
        ref = ref + A2.double() @ W2.double().t()
        args.update(A2=A2.to(DEV), W2=W2.to(DEV))
    out = ops.linear_fwd(**args)
    assert rel_err(out, ref) < 2e-6
    out = ops.linear_fwd(**args, scale=sc.to(DEV), shift=sh.to(DEV), relu=True)
    assert rel_err(out, torch.relu(ref * sc.double() + sh.double())) < 2e-6


@pytest.mark.parametrize("M,na,nb", [(5000, 128, 128), (333, 64, 28), (70000, 2, 64), (64, 130, 37)])
def test_linear_wgrad_and_colsum(M, na, nb):
    from dgnn_amd import ops
    g = torch.Generator().manual_seed(M)
    A, B = torch.randn(M, na, generator=g), torch.randn(M, nb, generator=g)
    dW = ops.linear_wgrad(A.to(DEV), B.to(DEV))
    assert rel_err(dW, A.double().t() @ B.double()) < 1e-5
    assert rel_err(ops.colsum(A.to(DEV)), A.double().sum(0)) < 1e-5


@pytest.mark.parametrize("M,na,nb1,nb2", [(5000, 128, 128, 128), (333, 64, 28, 28), (70000, 128, 64, 64), (64, 130, 37, 0), (2048, 64, 128, 0), (1, 2, 3, 3)])
def test_merged_weight_gradient_launch_matches_the_separate_calls(M, na, nb1, nb2):
    """dgnn_linear_wgrad_x3_cat: dW1 / dW2 bit for bit the two dgnn_linear_wgrad_x3 calls it replaces, the bias sums against fp64"""
    from dgnn_amd import ops
    if ops.GEMM_MODE == ops.GEMM_F32:
        pytest.skip("x3 arithmetic only")
    g = torch.Generator().manual_seed(M + nb2)
    A, B1 = torch.randn(M, na, generator=g).to(DEV), torch.randn(M, nb1 + 3, generator=g).to(DEV)[:, 3:]   # B1: a strided view
    B2 = torch.randn(M, nb2, generator=g).to(DEV) if nb2 else None
    dW1, dW2, db = ops.linear_wgrad_cat(A, B1, B2)
    assert torch.equal(dW1, ops.linear_wgrad(A, B1))
    if nb2:
        assert torch.equal(dW2, ops.linear_wgrad(A, B2))
    ref = A.double().sum(0)
    assert (db.double() - ref).abs().max().item() <= 1e-6 * A.double().abs().sum(0).max().item()
    dW1b, _, none = ops.linear_wgrad_cat(A, B1, B2, bias=False)
    assert none is None and torch.equal(dW1b, dW1)


@pytest.mark.parametrize("M,k1,k2,n_out", [(70001, 28, 28, 64), (30011, 64, 64, 128), (10007, 128, 128, 128), (2048, 128, 0, 64), (33, 128, 128, 128),
                                          (31, 64, 0, 2), (20000, 64, 64, 256), (50000, 64, 64, 256)])
def test_batch_statistics_from_the_gemm_epilogue(M, k1, k2, n_out):
    """dgnn_linear_fwd_x3_stats: z bit for bit dgnn_linear_fwd_x3's; mean / var / folded scale and shift equal to what dgnn_bn_batch_stats_fold
    derives from z (both sum in fp64; the orders differ, so a last-bit difference is possible at an exact rounding tie and tolerated)."""
    from dgnn_amd import ops
    from dgnn_amd._lib import lib
    if ops.GEMM_MODE == ops.GEMM_F32:
        pytest.skip("x3 arithmetic only")
    g = torch.Generator().manual_seed(M)
    A1, W1 = (torch.randn(M, k1, generator=g) * 2 + 0.3).to(DEV), torch.randn(n_out, k1, generator=g).to(DEV)
    A2 = torch.randn(M, k2, generator=g).to(DEV) if k2 else None
    W2 = torch.randn(n_out, k2, generator=g).to(DEV) if k2 else None
    bias, gamma, beta = torch.randn(n_out, generator=g).to(DEV), (torch.rand(n_out, generator=g) + 0.5).to(DEV), torch.randn(n_out, generator=g).to(DEV)
    got = ops.linear_fwd_with_batch_stats(A1, W1, A2, W2, bias, gamma, beta)
    big = n_out > 128 and -(-M // 256) * -(-n_out // 256) >= 192      # the 256 x 256 tile has no statistics epilogue (DGNN_X3_BIG=0: never taken)
    if got is None:
        assert big
        return
    assert not big or os.environ.get("DGNN_X3_BIG") == "0"
    z, mean, var, scale, shift = got
    z_ref = torch.empty_like(z)
    ops.check(lib().dgnn_linear_fwd_x3(ops.ptr(A1), k1, k1, ops.ptr(W1), k1, ops.ptr(A2), k2, k2, ops.ptr(W2), k2, ops.ptr(bias), None, None, 0, M, n_out,
                                       ops.ptr(z_ref), n_out, ops.stream_ptr()), "dgnn_linear_fwd_x3")
    assert torch.equal(z, z_ref)
    st = torch.empty(4, n_out, device=DEV)
    scratch = torch.empty(int(lib().dgnn_colstats_scratch_elems(M, n_out)), device=DEV)
    ops.check(lib().dgnn_bn_batch_stats_fold(ops.ptr(z_ref), n_out, M, n_out, ops.ptr(st[0]), ops.ptr(st[1]), None, None, 0.0, ops.ptr(gamma), ops.ptr(beta), 1e-5,
                                             ops.ptr(st[2]), ops.ptr(st[3]), ops.ptr(scratch), ops.stream_ptr()), "dgnn_bn_batch_stats_fold")
    for a, b in zip((mean, var, scale, shift), st):
        assert (a - b).abs().max().item() <= 2.4e-7 * b.abs().max().item()
    zd = z_ref.double()
    assert (mean.double() - zd.mean(0)).abs().max().item() < 1e-5 and (var.double() - zd.var(0, unbiased=False)).abs().max().item() < 1e-4 * zd.var(0).max().item()


@pytest.mark.parametrize("c_in,n_src,n_dst", [(64, 900, 600), (128, 5000, 1777), (28, 333, 333), (128, 40, 7)])
def test_aggregate_backward_with_addend_matches_the_two_steps(c_in, n_src, n_dst):
    """dgnn_sage_aggregate_bwd_add: dx = aggregate backward, then dx[:n_add] += add in one fp32 addition per element -- bit for bit; dWe / dbe
    untouched by the addend"""
    from dgnn_amd import ops
    g = torch.Generator().manual_seed(c_in + n_src)
    E = 4 * n_dst
    ei = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.arange(n_dst).repeat_interleave(4)])
    if n_src > 100:
        ei[0, : E // 3] = ei[0, : E // 3] % 50          # a few sources with dozens of out-edges, most of the others with none or a few
    x, da, ea = torch.randn(n_src, c_in, generator=g).to(DEV), torch.randn(n_dst, c_in, generator=g).to(DEV), torch.randn(E, 20, generator=g).to(DEV)
    We, be = (torch.randn(c_in, 20, generator=g) * 0.3).to(DEV), torch.randn(c_in, generator=g).to(DEV)
    rowptr, _, _ = ops.plan_build(ei.to(DEV), n_dst, 1)
    t_rowptr, t_dst, t_eid = ops.plan_build(ei.to(DEV), n_src, 0)
    n_add = n_dst if n_dst <= n_src else n_src
    wide = torch.randn(n_add, 2 * c_in, generator=g).to(DEV)
    add = wide[:, c_in:]                                 # the second half of a [n_dst, 2 c_in] GEMM output, as the training step passes it
    dx0, dWe0, dbe0, _ = ops.aggregate_bwd(t_rowptr, t_dst, t_eid, n_src, rowptr, x, da, ea, We, be)
    dx1, dWe1, dbe1 = ops.aggregate_bwd_add(t_rowptr, t_dst, t_eid, n_src, rowptr, x, da, ea, We, be, add)
    want = dx0.clone()
    want[:n_add] += add
    assert torch.equal(dx1, want)
    assert torch.equal(dWe1, dWe0) and torch.equal(dbe1, dbe0)


@pytest.mark.parametrize("c_in", [28, 64, 32, 48, 20])
@pytest.mark.parametrize("graph", ["tets", "thinned", "ragged", "tiny"])
def test_aggregate_backward_on_the_matrix_cores(c_in, graph):
    """k_agg_bwd_mm (round 6: rows of up to 64 channels; the filter's recomputation and dWe = dphi^T . [A | 1] as v_mfma_f32_16x16x4_f32, 4 out-edge
    slots per source row) against k_agg_bwd_c (taken when the row stride of x is no multiple of 2 / 4) and against fp64: dx bit for bit (the same
    chains: phi's bias-then-attributes fmaf chain, da / in-degree, the slot-ordered sum), dWe / dbe at fp32 rounding level of their sums (another
    order).  tets: every degree 4; thinned: degrees 0..4 (partly filled slots, in-degrees that are no power of two: the division); ragged: sources with
    dozens of out-edges (the per-edge path); tiny: a few dozen cells.  With and without dx, with the addend.  (DGNN_AGG_MFMA=0: both sides run k_agg_bwd_c.)"""
    from dgnn_amd import ops
    from dgnn_amd.synthetic import delaunay_tet_graph
    g = torch.Generator().manual_seed(c_in)
    adj, _, _ = delaunay_tet_graph(12 if graph == "tiny" else 700, seed=c_in)      # tiny: a few dozen cells -- one partly filled step
    n = adj.shape[0] // 4
    ei = torch.from_numpy(adj.T.astype(np.int64))
    if graph == "thinned":
        ei = ei[:, torch.rand(ei.size(1), generator=g) < 0.7]
    elif graph == "ragged":
        ei = ei.clone()
        ei[0, : ei.size(1) // 3] = ei[0, : ei.size(1) // 3] % 37
    E = ei.size(1)
    n_src = n_dst = n
    x, da, ea = torch.randn(n_src, c_in, generator=g), torch.randn(n_dst, c_in, generator=g), torch.randn(E, 20, generator=g)
    We, be = torch.randn(c_in, 20, generator=g) * 0.3, torch.randn(c_in, generator=g)
    add = torch.randn(n_dst - 5, c_in, generator=g)
    # fp64 reference through autograd
    xd, Wd, bd = x.double().requires_grad_(), We.double().requires_grad_(), be.double().requires_grad_()
    phi = ea.double() @ Wd.t() + bd
    deg = torch.bincount(ei[1], minlength=n_dst).clamp_min(1).double()
    a = torch.zeros(n_dst, c_in, dtype=torch.float64).index_add_(0, ei[1], xd[ei[0]] * phi) / deg[:, None]
    (a * da.double()).sum().backward()
    rowptr, _, _ = ops.plan_build(ei.to(DEV), n_dst, 1)
    t_rowptr, t_dst, t_eid = ops.plan_build(ei.to(DEV), n_src, 0)
    dev = lambda t: t.to(DEV)
    x_d, da_d, ea_d, We_d, be_d, add_d = dev(x), dev(da), dev(ea), dev(We), dev(be), dev(add)
    xw = torch.zeros(n_src, c_in + 1, device=DEV)
    xw[:, :c_in] = x_d
    dx_m, dWe_m, dbe_m, _ = ops.aggregate_bwd(t_rowptr, t_dst, t_eid, n_src, rowptr, x_d, da_d, ea_d, We_d, be_d)
    dx_c, dWe_c, dbe_c, _ = ops.aggregate_bwd(t_rowptr, t_dst, t_eid, n_src, rowptr, xw[:, :c_in], da_d, ea_d, We_d, be_d)
    assert torch.equal(dx_m, dx_c)
    assert rel_err(dx_m, xd.grad) < 2e-6
    for got, old, ref in ((dWe_m, dWe_c, Wd.grad), (dbe_m, dbe_c, bd.grad)):
        scale = ref.abs().max().item()
        assert (got.double().cpu() - ref).abs().max().item() <= 3e-6 * scale, graph
        assert (got - old).abs().max().item() <= 3e-6 * scale
    # no dx (the first layer's form): the same parameter gradients as with dx
    none, dWe_n, dbe_n, _ = ops.aggregate_bwd(t_rowptr, t_dst, t_eid, n_src, rowptr, x_d, da_d, ea_d, We_d, be_d, need_dx=False)
    assert none is None and torch.equal(dWe_n, dWe_m) and torch.equal(dbe_n, dbe_m)
    # the addend folded into the dx store
    dx_a, dWe_a, dbe_a = ops.aggregate_bwd_add(t_rowptr, t_dst, t_eid, n_src, rowptr, x_d, da_d, ea_d, We_d, be_d, add_d)
    want = dx_m.clone()
    want[:add_d.size(0)] += add_d
    assert torch.equal(dx_a, want) and torch.equal(dWe_a, dWe_m) and torch.equal(dbe_a, dbe_m)
    # twice the same bits (accumulators and slabs in a fixed order)
    dx_2, dWe_2, dbe_2, _ = ops.aggregate_bwd(t_rowptr, t_dst, t_eid, n_src, rowptr, x_d, da_d, ea_d, We_d, be_d)
    assert torch.equal(dx_2, dx_m) and torch.equal(dWe_2, dWe_m) and torch.equal(dbe_2, dbe_m)


def test_batchnorm_train_eval_and_backward():
    from dgnn_amd import functional as Fn
    g = torch.Generator().manual_seed(3)
    M, c = 4321, 96
    x = torch.randn(M, c, generator=g) * 2 + 0.5
    for training in (True, False):
        bn_ref = torch.nn.BatchNorm1d(c)
        with torch.no_grad():
            bn_ref.weight.copy_(torch.rand(c, generator=g) + 0.5)
            bn_ref.bias.copy_(torch.randn(c, generator=g))
            bn_ref.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
            bn_ref.running_var.copy_(torch.rand(c, generator=g) + 0.5)
        bn = torch.nn.BatchNorm1d(c)
        bn.load_state_dict(bn_ref.state_dict())
        bn = bn.to(DEV)
        bn_ref.train(training)
        bn.train(training)
        xr = x.clone().requires_grad_(True)
        xg = x.to(DEV).requires_grad_(True)
        G = torch.randn(M, c, generator=g)
        yr = torch.relu(bn_ref(xr))
        (yr * G).sum().backward()
        yg = Fn.batch_norm_act(xg, bn, relu=True)
        (yg * G.to(DEV)).sum().backward()
        assert rel_err(yg, yr) < 1e-5
        assert rel_err(xg.grad, xr.grad) < 2e-5
        assert rel_err(bn.weight.grad, bn_ref.weight.grad) < 2e-5
        assert rel_err(bn.bias.grad, bn_ref.bias.grad) < 2e-5
        assert rel_err(bn.running_mean, bn_ref.running_mean) < 1e-5
        assert rel_err(bn.running_var, bn_ref.running_var) < 1e-5
        assert int(bn.num_batches_tracked) == int(bn_ref.num_batches_tracked)


# ---- whole model: golden vectors --------------------------------------------------------------------
@pytest.mark.parametrize("fused,mode", [(True, 0), (True, 1), (True, 2), (True, 3), (True, 4), (False, 0), (False, 4)])
def test_inference_layer_golden_f2(fused, mode):
    from dgnn_amd import ops
    g = gold("static_f2_regular256.npz")
    net = hip_static()
    data = Config(x=torch.from_numpy(g["x"]).to(DEV), edge_attr=torch.from_numpy(g["edge_attr"]).to(DEV),
                  edge_index=torch.from_numpy(g["adjacencies"].T.astype(np.int64)).to(DEV))
    ops.FUSED_ENABLED = fused
    old_mode, ops.GEMM_MODE = ops.GEMM_MODE, mode
    try:
        logits = net.inference_layer(data)
    finally:
        ops.FUSED_ENABLED = True
        ops.GEMM_MODE = old_mode
    err = np.abs(logits.cpu().numpy() - g["logits"]).max()
    assert err <= TOL_LOGIT, err
    assert np.abs(logits.cpu().numpy().astype(np.float64) - g["logits64"]).max() <= TOL_LOGIT
    # arg-max (the in/out label) agrees wherever the margin exceeds the tolerance
    ref = g["logits"]
    margin = np.abs(ref[:, 0] - ref[:, 1]) > TOL_LOGIT
    assert np.array_equal(logits.cpu().numpy().argmax(1)[margin], ref.argmax(1)[margin])


def test_inference_layer_golden_f1_real_block():
    g = gold("static_f1_ignatius.npz")
    net = hip_static()
    data = Config(x=torch.from_numpy(g["x"]).to(DEV), edge_attr=torch.from_numpy(g["edge_attr"]).to(DEV),
                  edge_index=torch.from_numpy(g["edge_index"].astype(np.int64)).to(DEV))
    logits = net.inference_layer(data)
    assert np.abs(logits.cpu().numpy() - g["logits"]).max() <= TOL_LOGIT


def test_per_layer_activations_vs_oracle():
    """Every layer's output (not only the logits) against the oracle, heavy-tailed inputs."""
    from dgnn_amd.synthetic import delaunay_tet_graph
    adj, _, _ = delaunay_tet_graph(1500, seed=5)
    n = adj.shape[0] // 4
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n, 29, generator=g)
    x[::97] *= 40.0  # real standardised features reach 174 sigma
    ea = torch.randn(4 * n, 20, generator=g)
    ei = torch.from_numpy(adj.T.astype(np.int64))
    onet = oracle_static(dtype=torch.float64)
    trace = []
    with torch.no_grad():
        ref = onet.inference_layer(Config(x=x.double(), edge_attr=ea.double(), edge_index=ei), trace)
    net = hip_static()
    xs = x.to(DEV)[:, 1:]
    from dgnn_amd.graph import plan_for
    plan = plan_for(ei.to(DEV), n, n)
    h = xs
    t = dict(trace)
    for i in range(4):
        h = net._eval_layers_one(i, h, ea.to(DEV), plan)
        assert rel_err(h, t["relu%d" % i]) < 1e-5, i
    logits = net.inference_layer(Config(x=x.to(DEV), edge_attr=ea.to(DEV), edge_index=ei.to(DEV)))
    assert (logits.double().cpu() - ref).abs().max().item() <= TOL_LOGIT * max(1.0, ref.abs().max().item() / 8)


def test_train_forward_backward_golden_f3():
    g = gold("static_f3_train_blocks.npz")
    net = hip_static(train=True)
    d = f3_data(g)
    data = Config(all=Config(x=d.all.x.to(DEV), edge_attr=d.all.edge_attr.to(DEV)), batch_n_id=d.batch_n_id.to(DEV),
                  batch_adjs=[(a.to(DEV), e.to(DEV), s) for a, e, s in d.batch_adjs])
    logits = net(data)
    assert np.abs(logits.detach().cpu().numpy() - g["logits"]).max() <= TOL_LOGIT
    (logits * torch.from_numpy(g["G"]).to(DEV)).sum().backward()
    # biases feeding a train-mode BatchNorm have an analytically zero gradient (the reference holds
    # rounding noise there), so the error is measured against the tensor's own scale plus a floor
    # tied to the largest gradient in the model
    gmax = max(np.abs(g[k]).max() for k in g.files if k.startswith("grad."))
    for k, p in net.named_parameters():
        ref = g["grad." + k]
        err = np.abs(p.grad.cpu().numpy() - ref).max()
        assert err <= 2e-4 * np.abs(ref).max() + 2e-6 * gmax, (k, err, np.abs(ref).max(), gmax)
    for k, b in net.named_buffers():
        ref = g["buf." + k]
        err = np.abs(b.cpu().numpy().astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30)
        assert err < 1e-5, (k, err)


def test_batch_layer_and_layer_batch_schedules():
    g = gold("static_f3_train_blocks.npz")
    gb = gold("static_f3_batch_layer.npz")
    net = hip_static()
    d = f3_data(g)
    data_all = Config(x=d.all.x.to(DEV), edge_attr=d.all.edge_attr.to(DEV))
    loader = [(len(g["batch"]), d.batch_n_id, d.batch_adjs)]
    xo = net.inference_batch_layer(data_all, loader)
    assert np.abs(xo[torch.from_numpy(g["batch"]).to(DEV)].cpu().numpy() - gb["logits_rows"]).max() <= TOL_LOGIT
    # layer-major schedule on 1-hop blocks covering the whole graph == whole-graph inference_layer
    from oracle.pyg_semantics import neighbor_sampler_full
    ei = g["adjacencies"].T.astype(np.int64)
    n = g["x"].shape[0]
    loader1 = []
    for s in range(0, n, 512):
        b = np.arange(s, min(n, s + 512))
        n_id, adjs = neighbor_sampler_full(ei, n, b, 1)
        a, e, size = adjs[0]
        loader1.append((len(b), torch.from_numpy(n_id), (torch.from_numpy(a), torch.from_numpy(e), size)))
    full = net.inference_layer(Config(x=data_all.x, edge_attr=data_all.edge_attr, edge_index=torch.from_numpy(ei).to(DEV)))
    lb = net.inference_layer_batch(data_all, loader1)
    assert (full - lb).abs().max().item() <= TOL_LOGIT


@pytest.mark.parametrize("points,heavy", [(12, False), (333, False), (3000, True)])
def test_last_layer_and_decoder_in_one_launch(points, heavy):
    """dgnn_sage_layer_fused_decoder_fwd (the last conv layer's launch carries Linear-BN-ReLU-Linear and writes logits, reference :180-187 / :350-351):
    against the oracle, against the two-launch form, on graphs smaller than a tile and not a multiple of one, with heavy-tailed inputs (the
    per-slab power-of-two scales), and in destination sub-ranges (bit-identical to the whole launch, as a partitioned scene needs)."""
    from dgnn_amd import ops
    from dgnn_amd.graph import GraphPlan
    from dgnn_amd.synthetic import delaunay_tet_graph
    net = hip_static()
    if ops.GEMM_MODE != ops.GEMM_F16X2 or not ops.FUSE_DECODER:
        pytest.skip("the one-launch form exists for the default arithmetic only (DGNN_GEMM_MODE / DGNN_FUSE_DECODER select the two-launch form)")
    assert net.fuses_decoder(3) and not net.fuses_decoder(2)
    adj, _, _ = delaunay_tet_graph(points, seed=points)
    n = adj.shape[0] // 4
    g = torch.Generator().manual_seed(points)
    x, ea = torch.randn(n, 29, generator=g), torch.randn(4 * n, 20, generator=g)
    if heavy:
        x[::17] *= 40.0
        ea[::23] *= 25.0
    ei = torch.from_numpy(adj.T.astype(np.int64))
    with torch.no_grad():
        ref = oracle_static().inference_layer(Config(x=x, edge_attr=ea, edge_index=ei))
    data = Config(x=x.to(DEV), edge_attr=ea.to(DEV), edge_index=ei.to(DEV))
    one = net.inference_layer(data)
    old, ops.FUSE_DECODER = ops.FUSE_DECODER, False
    try:
        assert not net.fuses_decoder(3)
        two = net.inference_layer(data)
    finally:
        ops.FUSE_DECODER = old
    tol = TOL_LOGIT * max(1.0, ref.abs().max().item())
    assert (one.cpu() - ref).abs().max().item() <= tol and (two.cpu() - ref).abs().max().item() <= tol
    assert (one - two).abs().max().item() <= 0.3 * tol
    assert torch.equal(one, net.inference_layer(data))                       # run to run
    # destination sub-ranges of the last layer (interior / boundary launches of a partition): the same logits bit for bit
    plan = GraphPlan(data.edge_index, n, n)
    h = data.x[:, 1:]
    for i in range(3):
        h = net._eval_layers(h, n, data.edge_attr, [plan] * 4, True, only=i)
    cut = [0, n // 3, n // 3 + 1, n]
    out = torch.full((n, 2), float("nan"), device=DEV)
    for b, e in zip(cut[:-1], cut[1:]):
        net._eval_layers(h, n, data.edge_attr, [plan] * 4, True, only=3, out=out, rows=(b, e), decode=True)
    assert torch.equal(out, one)


def test_prepared_parameters_give_the_same_bits_and_follow_the_weights():
    """dgnn_sage_layer_prepare + the *_p entry points (the launch reads the scales / split filter operand / resident weight fragments / decoder
    fragments instead of deriving them): bit-identical to the launches that derive them, for every fused shape of the shipped model and for the
    launch that carries the decoder; the cache follows in-place updates of the weights (version counters) and load_state_dict."""
    from dgnn_amd import ops
    from dgnn_amd.synthetic import delaunay_tet_graph
    if ops.GEMM_MODE != ops.GEMM_F16X2:
        pytest.skip("prepared parameters exist for the default arithmetic")
    adj, _, _ = delaunay_tet_graph(1500, seed=2)
    n = adj.shape[0] // 4
    g = torch.Generator().manual_seed(4)
    data = Config(x=torch.randn(n, 29, generator=g).to(DEV), edge_attr=torch.randn(4 * n, 20, generator=g).to(DEV),
                  edge_index=torch.from_numpy(adj.T.astype(np.int64)).to(DEV))
    net = hip_static()
    old = ops.PREPARED_PARAMS
    try:
        ops.PREPARED_PARAMS = False
        plain = net.inference_layer(data)
        ops.PREPARED_PARAMS = True
        prep = net.inference_layer(data)
        assert torch.equal(plain, prep)
        cache = net.__dict__["_prep_cache"]
        last = (3, bool(ops.FUSE_DECODER))        # DGNN_FUSE_DECODER=0: the last layer is a plain launch too
        assert sorted(cache) == [(0, False), (1, False), (2, False), last] and all(v[1] is not None for v in cache.values())
        bufs = {k: v[1].data_ptr() for k, v in cache.items()}
        assert torch.equal(net.inference_layer(data), prep) and {k: v[1].data_ptr() for k, v in cache.items()} == bufs      # cache hit: nothing re-made
        # an in-place update of one layer's weights re-prepares that layer only, and the result follows the new weights
        with torch.no_grad():
            net.convs[1][0].lin_j.weight.mul_(1.5)
        upd = net.inference_layer(data)
        ops.PREPARED_PARAMS = False
        assert torch.equal(upd, net.inference_layer(data)) and not torch.equal(upd, prep)
        ops.PREPARED_PARAMS = True
        # each layer on its own, sub-ranges included (the partitioned forward's launches)
        from dgnn_amd.graph import GraphPlan
        plan = GraphPlan(data.edge_index, n, n)
        h = data.x[:, 1:]
        for i in range(4):
            outs = []
            for flag in (False, True):
                ops.PREPARED_PARAMS = flag
                dec = i == 3 and net.fuses_decoder(3)          # (DGNN_FUSE_DECODER=0: the last layer writes its rows like the others)
                o = torch.full((n, 2 if dec else net.convs[i][0].lin_j.out_features), float("nan"), device=DEV)
                for b, e in ((0, n // 2), (n // 2, n)):
                    net._eval_layers(h, n, data.edge_attr, [plan] * 4, True, only=i, out=o, rows=(b, e), decode=dec)
                outs.append(o)
            assert torch.equal(outs[0], outs[1]), i
            if i < 3:
                h = outs[0]
    finally:
        ops.PREPARED_PARAMS = old


def test_other_widths_random_init():
    """[64,128,256,512] (configs/aerial.yaml:57) exercises the non-fused path and wide channel tiling."""
    from oracle.static_edge_filters import SurfaceNet as ONet
    from dgnn_amd.synthetic import delaunay_tet_graph
    convs = (64, 128, 256, 512)
    torch.manual_seed(0)
    onet = ONet(reconbench_pretrained(device="cpu", convs=convs)).eval()
    net = hip_static(convs=convs, sd=onet.state_dict())
    adj, _, _ = delaunay_tet_graph(500, seed=8)
    n = adj.shape[0] // 4
    g = torch.Generator().manual_seed(2)
    x, ea = torch.randn(n, 29, generator=g), torch.randn(4 * n, 20, generator=g)
    ei = torch.from_numpy(adj.T.astype(np.int64))
    with torch.no_grad():
        ref = onet.inference_layer(Config(x=x, edge_attr=ea, edge_index=ei))
    logits = net.inference_layer(Config(x=x.to(DEV), edge_attr=ea.to(DEV), edge_index=ei.to(DEV)))
    assert (logits.cpu() - ref).abs().max().item() <= TOL_LOGIT


@pytest.mark.parametrize("world", [2, 4])
def test_partitioned_hip_forward_equals_whole_graph(world):
    """Spatially partitioned forward with the HIP layers, ranks emulated in one process (the box has a
    single GPU): per layer every part runs on its local bipartite graph (n_src = own + halo), then halo
    rows are filled from their owners' outputs exactly as the RCCL exchange delivers them.  The union
    must equal the whole-graph result bit for bit (same kernels, same per-destination edge order)."""
    from dgnn_amd.graph import GraphPlan
    from dgnn_amd.partition import build_local_part, rcb_partition
    from dgnn_amd.synthetic import delaunay_tet_graph, hashed_normal
    adj, cent, _ = delaunay_tet_graph(4000, seed=6)
    n = adj.shape[0] // 4
    ei = adj.T.astype(np.int64)
    x = hashed_normal(np.arange(n), 29, seed=1, device=DEV)
    ea = hashed_normal(np.arange(4 * n), 20, seed=2, device=DEV)
    net = hip_static()
    full = net.inference_layer(Config(x=x, edge_attr=ea, edge_index=torch.from_numpy(ei).to(DEV)))
    part = rcb_partition(cent, world)
    lps = [build_local_part(ei, part, r, world) for r in range(world)]
    plans = [GraphPlan(torch.from_numpy(lp.edge_index).to(DEV), lp.n_own + lp.n_halo, lp.n_own) for lp in lps]
    for lp, pl in zip(lps, plans):   # local lists are grouped by destination: the plan is the identity
        assert torch.equal(pl.eid.cpu(), torch.arange(pl.E, dtype=torch.int32))
    eas = [ea[torch.from_numpy(lp.edge_gid).to(DEV)] for lp in lps]     # already in plan order
    hs = [x[torch.from_numpy(np.concatenate([lp.own_gid, lp.halo_gid])).to(DEV)][:, 1:] for lp in lps]
    widths = [64, 128, 128, 128]
    fuse = net.fuses_decoder(3)        # the last layer's launches then carry the decoder and write logits (as PartitionedScene.inference_layer runs them)
    for i in range(net.num_layers):
        bufs = []
        for r, lp in enumerate(lps):
            # as run_partitioned_layers does: interior cells, then (after the halo landed) boundary cells, as two launches
            dec = fuse and i == 3
            buf = torch.full((lp.n_own, 2) if dec else (lp.n_own + lp.n_halo, widths[i]), float("nan"), device=DEV)
            for b, e in ((0, lp.n_interior), (lp.n_interior, lp.n_own)):
                net._eval_layers(hs[r], lp.n_own, eas[r], [plans[r]] * 4, False, only=i, out=buf, rows=(b, e), decode=dec)
            bufs.append(buf)
        if fuse and i == 3:
            hs = bufs
            break
        glob = torch.empty(n, widths[i], device=DEV)
        for r in range(world):
            glob[torch.from_numpy(lps[r].own_gid).to(DEV)] = bufs[r][:lps[r].n_own]
        for r in range(world):           # what the exchange delivers
            bufs[r][lps[r].n_own:] = glob[torch.from_numpy(lps[r].halo_gid).to(DEV)]
        hs = bufs
    logits = torch.empty(n, 2, device=DEV)
    for r in range(world):
        logits[torch.from_numpy(lps[r].own_gid).to(DEV)] = hs[r] if fuse else net._eval_decoder(hs[r][:lps[r].n_own])
    assert torch.equal(logits, full)


def test_updated_variant_forward_backward_golden():
    from dgnn_amd.learning.surfaceNetUpdatedEdgeFilters import SurfaceNet
    g = gold("static_f3_train_blocks.npz")
    u = gold("updated_f3_blocks.npz")
    d = f3_data(g)
    for tag, name in (("plus", "sage+"), ("plain", "sage")):
        clf = Config.wrap(dict(training=dict(model_params=[int(v) for v in u[tag + ".model_params"]], model_name=name, loss="kl"),
                               features=dict(normalization_feature=1, keep_normalization_feature=0), temp=dict(device=DEV)))
        net = SurfaceNet(28, clf)
        net.load_state_dict({k[len(tag) + 7:]: torch.from_numpy(u[k]) for k in u.files if k.startswith(tag + ".param.")})
        net = net.to(DEV)
        data = Config(x=d.all.x.to(DEV), edge_attr=d.all.edge_attr.to(DEV), n_id=d.batch_n_id.to(DEV),
                      adjs=[(a.to(DEV), e.to(DEV), s) for a, e, s in d.batch_adjs])
        logits = net(data)
        ref = u[tag + ".logits"]
        assert np.abs(logits.detach().cpu().numpy() - ref).max() <= TOL_LOGIT * max(1.0, np.abs(ref).max())
        # our "+" head is also differentiable (the reference's raises there); grads are checked on "plain"
        (logits * torch.from_numpy(g["G"]).to(DEV)).sum().backward()
        if tag == "plain":
            gmax = max(np.abs(u[k]).max() for k in u.files if k.startswith("plain.grad."))
            for k, p in net.named_parameters():
                r = u["plain.grad." + k]
                err = np.abs(p.grad.cpu().numpy() - r).max()
                assert err <= 2e-4 * np.abs(r).max() + 2e-6 * gmax, (k, err, np.abs(r).max())


def test_partitioned_scene_world1_matches_inference_layer():
    from dgnn_amd.partition import PartitionedScene
    from dgnn_amd.synthetic import delaunay_tet_graph, hashed_normal
    net = hip_static()
    from dgnn_amd.synthetic import loader_cell_order
    scene = PartitionedScene.build_synthetic(1500, 3, 0, 1, DEV)
    logits = scene.inference_layer(net)
    adj, cent, _ = delaunay_tet_graph(1500, 3)
    adj = loader_cell_order(adj, cent)[0]          # build_synthetic numbers the cells the way the package's loader leaves a scene (ingest-time Morton order)
    n = adj.shape[0] // 4
    data = Config(x=hashed_normal(np.arange(n), 29, seed=1, device=DEV), edge_attr=hashed_normal(np.arange(4 * n), 20, seed=2, device=DEV),
                  edge_index=torch.from_numpy(adj.T.astype(np.int64)).to(DEV))
    assert torch.equal(logits, net.inference_layer(data))


def _two_rank_worker(rank, world, port, out_dir):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dgnn_amd.partition import PartitionedScene
    net = hip_static()
    scene = PartitionedScene.build_synthetic(6000, 5, rank, world, DEV)
    ex, lp = scene.exchange, scene.lp
    assert ex.stream is not None and lp.n_interior > 0 and lp.n_halo > 0

    # both ranks share the box's single GPU (RCCL wants one GPU per rank): under gloo the exchange stages the rows through
    # host memory; the stream choreography -- pack on the compute stream, transfer on the side stream, interior launch in
    # between, boundary launch after wait() -- is the same as with RCCL
    assert ex.via_host
    for _ in range(3):  # several steps: buffers are recycled by the allocator across streams
        logits = scene.inference_layer(net)
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "r%d.npz" % rank), gid=lp.own_gid, logits=logits.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_partitioned_scene_two_processes_overlapped_exchange(world, tmp_path):
    """PartitionedScene.inference_layer end to end in several processes (interior launch || exchange on a side stream,
    boundary launch after the wait), union of the ranks' logits == whole-graph inference_layer, bit for bit."""
    import socket
    import torch.multiprocessing as mp
    from dgnn_amd.synthetic import delaunay_tet_graph, hashed_normal
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    mp.spawn(_two_rank_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    from dgnn_amd.synthetic import loader_cell_order
    adj, cent, _ = delaunay_tet_graph(6000, 5)
    adj = loader_cell_order(adj, cent)[0]          # (build_synthetic's cell numbering: the loader's ingest-time order)
    n = adj.shape[0] // 4
    data = Config(x=hashed_normal(np.arange(n), 29, seed=1, device=DEV), edge_attr=hashed_normal(np.arange(4 * n), 20, seed=2, device=DEV),
                  edge_index=torch.from_numpy(adj.T.astype(np.int64)).to(DEV))
    ref = hip_static().inference_layer(data).cpu().numpy()
    got = np.full_like(ref, np.nan)
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), "r%d.npz" % r))
        got[d["gid"]] = d["logits"]
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("M,n_out", [(1000, 2), (64, 2), (4097, 1), (1, 2)])
def test_decoder_fused(M, n_out):
    from dgnn_amd import ops
    g = torch.Generator().manual_seed(M + n_out)
    y = torch.randn(M, 128, generator=g)
    W0, b0 = torch.randn(64, 128, generator=g) * 0.2, torch.randn(64, generator=g)
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    W3, b3 = torch.randn(n_out, 64, generator=g) * 0.3, torch.randn(n_out, generator=g)
    ref = torch.relu((y.double() @ W0.double().t() + b0.double()) * sc.double() + sh.double()) @ W3.double().t() + b3.double()
    out = ops.decoder_fused_fwd(*(t.to(DEV) for t in (y, W0, b0, sc, sh, W3, b3)))
    assert rel_err(out, ref) < 3e-6


@pytest.mark.parametrize("c_in,c_out", [(28, 64), (64, 128), (128, 128), (20, 128), (64, 64)])
def test_fused_layer_gemm_modes_vs_fp64(c_in, c_out):
    """The fused layer in exact-fp32 MFMA mode and in split-bf16 (3x3 -> 6 products) mode against an fp64
    evaluation: both must sit at fp32 rounding level (the split mode drops only terms <= 2^-25 relative)."""
    from dgnn_amd import ops
    from dgnn_amd.graph import GraphPlan
    from dgnn_amd.synthetic import delaunay_tet_graph
    from oracle.pyg_semantics import propagate_mean
    adj, _, _ = delaunay_tet_graph(1200, seed=c_in)
    n = adj.shape[0] // 4
    ei = torch.from_numpy(adj.T.astype(np.int64))
    g = torch.Generator().manual_seed(c_out)
    x = torch.randn(n, c_in, generator=g) * torch.exp(torch.randn(n, 1, generator=g))  # wide dynamic range
    ea = torch.randn(4 * n, 20, generator=g)
    We, be = torch.randn(c_in, 20, generator=g) * 0.3, torch.randn(c_in, generator=g)
    Wj, Wi, bj = torch.randn(c_out, c_in, generator=g) * 0.2, torch.randn(c_out, c_in, generator=g) * 0.2, torch.randn(c_out, generator=g)
    sc, sh = torch.rand(c_out, generator=g) + 0.5, torch.randn(c_out, generator=g)
    phi = ea.double() @ We.double().t() + be.double()
    a = propagate_mean(x.double(), n, ei, phi)
    ref = torch.relu((a @ Wj.double().t() + bj.double() + x.double() @ Wi.double().t()) * sc.double() + sh.double())
    plan = GraphPlan(ei.to(DEV), n, n)
    eas = plan.sorted_edge_attr(ea.to(DEV))
    errs = {}
    for mode in (ops.GEMM_F32, ops.GEMM_BF16X3, ops.GEMM_BF16X3_FILTER, ops.GEMM_F16X2_DENSE, ops.GEMM_F16X2):
        out = ops.sage_layer_fused_fwd(plan.rowptr, plan.src, n, x.to(DEV), eas, We.to(DEV), be.to(DEV), Wj.to(DEV), bj.to(DEV),
                                       Wi.to(DEV), sc.to(DEV), sh.to(DEV), True, gemm_mode=mode)
        errs[mode] = rel_err(out, ref)
        assert errs[mode] < 3e-6, (mode, errs)
        # same launch reading the caller's edge_attr in place (rows DMA-gathered by eid): identical bits
        out_g = ops.sage_layer_fused_fwd(plan.rowptr, plan.src, n, x.to(DEV), ea.to(DEV), We.to(DEV), be.to(DEV), Wj.to(DEV),
                                         bj.to(DEV), Wi.to(DEV), sc.to(DEV), sh.to(DEV), True, gemm_mode=mode, eid=plan.eid)
        assert torch.equal(out_g, out), mode
    assert errs[ops.GEMM_BF16X3] < 3 * errs[ops.GEMM_F32] + 2e-7, errs
    assert errs[ops.GEMM_BF16X3_FILTER] < 3 * errs[ops.GEMM_F32] + 2e-7, errs
    # fp16 x 2 (22 significand bits per operand, lo.lo dropped): within a small multiple of the fp32 chain's own rounding
    print("fused %d->%d rel. err vs fp64 by mode:" % (c_in, c_out), {k: "%.2e" % v for k, v in errs.items()})
    assert errs[ops.GEMM_F16X2_DENSE] < 4 * errs[ops.GEMM_F32] + 2e-7, errs
    assert errs[ops.GEMM_F16X2] < 4 * errs[ops.GEMM_F32] + 2e-7, errs


@pytest.mark.parametrize("c_in,c_out,sliced", [(28, 64, False), (28, 64, True), (29, 64, False), (64, 128, False), (128, 128, False), (64, 64, False), (32, 128, True),
                                               (64, 128, True)])
def test_f32_filter_product_on_the_matrix_cores_is_the_fmaf_chain(c_in, c_out, sliced):
    """gemm_mode f32 (round 6): the 4-regular fast path computes phi = We . A + be on v_mfma_f32_16x16x4_f32 (C input = the bias, attributes ascending);
    the per-edge path of the same kernel (a wave whose group of tets crosses n_dst) runs the fmaf chain on the VALU from the same start in the same
    order.  Cutting n_dst short by 1..7 rows moves the rows in front of the cut from the first path to the second: not a bit may change, in them or
    anywhere else.  (DGNN_FILTER_MFMA=0 runs both on the VALU.)"""
    from dgnn_amd import ops
    n, ei, plan, t = _fused_case(900, c_in, c_out, seed=c_in + c_out)
    d = {k: v.to(DEV) for k, v in t.items()}
    if sliced:      # rows behind a column slice, as the scene's feature rows are (x[:, 1:]): neither 8- nor 16-byte aligned (dword loads / the VALU form)
        d["x"] = torch.cat([torch.zeros(n, 1), t["x"]], 1).to(DEV)[:, 1:]
    def run(n_dst):
        return ops.sage_layer_fused_fwd(plan.rowptr, plan.src, n_dst, d["x"], d["ea"], d["We"], d["be"], d["Wj"], d["bj"], d["Wi"], None, None, False,
                                        gemm_mode=ops.GEMM_F32, eid=plan.eid)
    whole = run(n)
    assert rel_err(whole, _fused_ref(n, ei, t)) < 3e-6
    for cut in range(1, 8):
        part = run(n - cut)
        assert part.shape[0] == n - cut and torch.equal(part, whole[:n - cut]), cut


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_fused_layers_row_level_on_larger_graph(mode):
    """Row-level check of every fused layer on a 134k-tet graph (thousands of tiles per launch, several launches) in every
    matrix-core mode, the default (4 = f16x2) included: EVERY output row of every layer against the ORACLE's trace of the same
    layer (CPU, fp32) -- not against another HIP path.  This is the detector that caught a rare single-row race in an abandoned
    wave-specialised variant (tools/dbg_rows.py); each layer is launched four times on the oracle's input of that layer."""
    from dgnn_amd import ops
    from dgnn_amd.graph import GraphPlan
    from dgnn_amd.synthetic import delaunay_tet_graph, hashed_normal
    net = hip_static()
    adj, _, _ = delaunay_tet_graph(20000, 3)
    n = adj.shape[0] // 4
    x = hashed_normal(np.arange(n), 29, seed=1, device="cpu")
    ea = hashed_normal(np.arange(4 * n), 20, seed=2, device="cpu")
    ei = torch.from_numpy(adj.T.astype(np.int64))
    trace = []
    with torch.no_grad():
        oracle_static().inference_layer(Config(x=x, edge_attr=ea, edge_index=ei), trace)
    acts = [x[:, 1:].contiguous().to(DEV)] + [v.to(DEV) for k, v in trace if k.startswith("relu")]
    assert len(acts) == 5
    ea_d = ea.to(DEV)
    plan = GraphPlan(ei.to(DEV), n, n)
    old, ops.GEMM_MODE = ops.GEMM_MODE, mode
    try:
        for i in range(4):
            ref = acts[i + 1]
            for rep in range(4):
                o = net._eval_layers(acts[i].clone(), n, ea_d, [plan] * 4, True, only=i)
                bad = ((o - ref).abs() > 2e-5 * ref.abs().max()).any(1).nonzero().flatten()
                assert bad.numel() == 0, (i, rep, bad[:8].tolist(), float((o - ref).abs().max()))
    finally:
        ops.GEMM_MODE = old


@pytest.mark.parametrize("variant", ["edge_convs0", "edge_convs2", "decoder1", "loss_bce", "loss_mse"])
def test_config_variants_vs_oracle(variant):
    """Configuration branches of SurfaceNet.__init__ (surfaceNetStaticEdgeFilters.py:104-187) that no shipped YAML takes: lin_e with 0 / 2
    layers, the one-Linear decoder, output_dim 1 (bce / mse).  Random-initialised oracle model -> same state_dict in the HIP model ->
    inference_layer and a train-mode forward/backward on sampled blocks."""
    from oracle.static_edge_filters import SurfaceNet as ONet
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import SurfaceNet
    from dgnn_amd.synthetic import delaunay_tet_graph
    from oracle.pyg_semantics import neighbor_sampler_full

    def clf_for(device):
        clf = reconbench_pretrained(device=device)
        if variant.startswith("edge_convs"):
            clf.model.edge_convs = int(variant[-1])
        elif variant == "decoder1":
            clf.model.decoder = 1
        else:
            clf.training.loss = variant.split("_")[1]
        return clf
    torch.manual_seed(11)
    try:
        onet = ONet(clf_for("cpu"))
    except SystemExit:
        with pytest.raises(SystemExit):      # a combination the reference itself refuses: the product must refuse it the same way
            SurfaceNet(clf_for(DEV))
        return
    net = SurfaceNet(clf_for(DEV))
    net.load_state_dict(onet.state_dict(), strict=True)
    net = net.to(DEV)
    adj, _, _ = delaunay_tet_graph(700, seed=4)
    n = adj.shape[0] // 4
    g = torch.Generator().manual_seed(5)
    x, ea = torch.randn(n, 29, generator=g), torch.randn(4 * n, 20, generator=g)
    ei = torch.from_numpy(adj.T.astype(np.int64))
    onet.eval(), net.eval()
    with torch.no_grad():
        ref = onet.inference_layer(Config(x=x, edge_attr=ea, edge_index=ei))
    got = net.inference_layer(Config(x=x.to(DEV), edge_attr=ea.to(DEV), edge_index=ei.to(DEV)))
    assert got.shape == ref.shape
    assert (got.cpu() - ref).abs().max().item() <= TOL_LOGIT * max(1.0, ref.abs().max().item())
    # train-mode forward / backward on 4-hop blocks
    n_id, adjs = neighbor_sampler_full(adj.T.astype(np.int64), n, np.arange(40), 4)
    onet.train(), net.train()
    od = Config(all=Config(x=x, edge_attr=ea), batch_n_id=torch.from_numpy(n_id),
                batch_adjs=[(torch.from_numpy(a), torch.from_numpy(e), s) for a, e, s in adjs])
    hd = Config(all=Config(x=x.to(DEV), edge_attr=ea.to(DEV)), batch_n_id=torch.from_numpy(n_id).to(DEV),
                batch_adjs=[(torch.from_numpy(a).to(DEV), torch.from_numpy(e).to(DEV), s) for a, e, s in adjs])
    ol, hl = onet(od), net(hd)
    G = torch.randn(ol.shape, generator=g)
    (ol * G).sum().backward()
    (hl * G.to(DEV)).sum().backward()
    assert (hl.detach().cpu() - ol.detach()).abs().max().item() <= 2e-4 * max(1.0, ol.abs().max().item())
    og = dict(onet.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in og.values() if p.grad is not None)
    for k, p in net.named_parameters():
        if og[k].grad is None:
            assert p.grad is None or p.grad.abs().max().item() == 0, k
            continue
        d = (p.grad.cpu() - og[k].grad).abs().max().item()
        assert d <= 5e-4 * og[k].grad.abs().max().item() + 5e-6 * gmax, (k, d)


@pytest.mark.parametrize("hops", [1, 4])
def test_gpu_block_builder_matches_neighbor_sampler(hops):
    """GPU k-hop block builder == the oracle's restatement of PyG NeighborSampler(sizes=[-1]*k): n_id, local edge
    lists, e_id and sizes, integer-exact, over consecutive batches (state is reset between them)."""
    from dgnn_amd.sampler import NeighborSampler
    from dgnn_amd.synthetic import delaunay_tet_graph
    from oracle.pyg_semantics import neighbor_sampler_full
    adj, _, _ = delaunay_tet_graph(700, seed=12)
    n = adj.shape[0] // 4
    ei = adj.T.astype(np.int64)
    rng = np.random.default_rng(3)
    node_idx = torch.from_numpy(rng.permutation(n)[:300].astype(np.int64))
    loader = NeighborSampler(torch.from_numpy(ei).to(DEV), sizes=[-1] * hops, node_idx=node_idx, num_nodes=n, batch_size=128)
    assert len(loader) == 3
    for k, (bs, n_id, adjs) in enumerate(loader):
        b = node_idx[k * 128:(k + 1) * 128].numpy()
        ref_n_id, ref_adjs = neighbor_sampler_full(ei, n, b, hops)
        assert bs == len(b) and np.array_equal(n_id.cpu().numpy(), ref_n_id)
        adjs = [adjs] if hops == 1 else adjs
        for (e, eid, size), (re, reid, rsize) in zip(adjs, ref_adjs):
            assert tuple(size) == tuple(rsize)
            assert np.array_equal(e.cpu().numpy(), re) and np.array_equal(eid.cpu().numpy(), reid)
    # blocks drive the model: batch-major inference on GPU-built blocks == whole-graph inference
    net = hip_static()
    g = torch.Generator().manual_seed(1)
    x, ea = torch.randn(n, 29, generator=g).to(DEV), torch.randn(4 * n, 20, generator=g).to(DEV)
    if hops == 4:
        full = net.inference_layer(Config(x=x, edge_attr=ea, edge_index=torch.from_numpy(ei).to(DEV)))
        xo = net.inference_batch_layer(Config(x=x, edge_attr=ea), loader)
        sel = node_idx.to(DEV)
        assert (xo[sel] - full[sel]).abs().max().item() <= TOL_LOGIT


def test_trainer_shim_trains_on_gpu_blocks():
    """End-to-end training slice on the GPU: blocks from the GPU sampler -> SurfaceNet.forward (HIP, BN train mode)
    -> runModel-style KL loss weighted by volume -> backward through the HIP kernels -> Adam.  The first step's loss
    must equal the oracle's on the same batch, and the loss must go down over a few steps."""
    from dgnn_amd.learning.runModel import Metrics, Trainer, adjust_learning_rate
    from dgnn_amd.sampler import NeighborSampler
    from dgnn_amd.synthetic import delaunay_tet_graph
    from oracle.pyg_semantics import neighbor_sampler_full
    adj, _, _ = delaunay_tet_graph(600, seed=21)
    n = adj.shape[0] // 4
    ei = torch.from_numpy(adj.T.astype(np.int64))
    g = torch.Generator().manual_seed(4)
    x = torch.randn(n, 29, generator=g)
    x[:, 0] = x[:, 0].abs() + 0.05
    ea = torch.randn(4 * n, 20, generator=g)
    occ = torch.sigmoid(2 * x[:, 3:4] + x[:, 7:8])
    y = torch.cat([occ, 1 - occ], 1)
    clf = reconbench_pretrained(device=DEV)
    clf.temp.current_epoch = 0
    clf.training.metrics = Metrics()
    net = hip_static(train=True)
    tr = Trainer(net)
    opt = torch.optim.Adam(net.parameters(), lr=clf.training.learning_rate)
    adjust_learning_rate(opt, clf)
    loader = NeighborSampler(ei.to(DEV), sizes=[-1] * 4, node_idx=torch.arange(0, n, 3), num_nodes=n, batch_size=256)
    all_ = Config(x=x.to(DEV), y=y.to(DEV), edge_attr=ea.to(DEV))
    losses = []
    first = None
    for epoch in range(3):
        for bs, n_id, adjs in loader:
            data = Config(all=all_, batch_n_id=n_id, batch_adjs=adjs)
            if first is None:
                first = (n_id.cpu(), [(a.cpu(), e.cpu(), s) for a, e, s in adjs])
                onet = oracle_static(train=True)
                od = Config(all=Config(x=x, edge_attr=ea), batch_n_id=first[0], batch_adjs=first[1])
                ol = onet(od)
                ids = first[0][:first[1][-1][2][1]]
                l = F_kl(ol, y[ids], x[ids, 0])
            losses.append(float(tr.train(data, opt, clf)))
            if len(losses) == 1:
                assert abs(losses[0] - l) <= 1e-4 * max(1.0, abs(l)), (losses[0], l)
    assert losses[-1] < 0.7 * losses[0], losses
    assert clf.training.metrics.getOA() > 50


def F_kl(logits, gt, vol):
    import torch.nn.functional as F
    cl = F.kl_div(F.log_softmax(logits, dim=-1), gt[:, :2], reduction='none').sum(1) * vol
    return float((cl.sum() / vol.sum()).detach())


def test_interface_extraction_matches_reference_loops():
    """Device label/interface extraction vs a direct restatement of processing/generate_mesh.py:75,93-105."""
    from dgnn_amd.processing.generate_mesh import extract_interface
    rng = np.random.default_rng(5)
    n, nf_facets = 5000, 9000
    infinite = (rng.random(n) < 0.05).astype(np.int32)
    logits = rng.standard_normal((n, 2)).astype(np.float32)
    logits[::50] = 0.25  # exact ties -> class 0, as argmax does
    n_fin = int((infinite == 0).sum())
    nfacets = rng.integers(-1, n_fin, size=(nf_facets, 2)).astype(np.int32)
    # reference semantics
    labels = torch.log_softmax(torch.from_numpy(logits)[torch.from_numpy(infinite) == 0], dim=-1).argmax(1).numpy()
    edges = nfacets.copy()
    edges[edges == -1] = labels.shape[0]
    lab = np.append(labels, 1)
    interfaces = [fi for fi, f in enumerate(edges) if lab[f[0]] != lab[f[1]]]
    got_labels, got_if = extract_interface(torch.from_numpy(logits).to(DEV), torch.from_numpy(infinite).to(DEV), torch.from_numpy(nfacets).to(DEV))
    assert np.array_equal(got_labels.cpu().numpy(), labels)
    assert np.array_equal(got_if.cpu().numpy(), np.asarray(interfaces, dtype=np.int32))


@pytest.mark.parametrize("fix", [0, 1])
def test_generate_matches_the_reference_run(tmp_path, fix):
    """processing/generate_mesh.generate(data, prediction, clf) against what the REFERENCE's generate handed to trimesh.Trimesh on the same inputs
    (tests/golden/genmesh_f4_small.npz, make_golden.py round3: graph cut off / unavailable, exact ties in the logits, hull facets with the
    infinite cell on one side): same vertices, same interface triangles in the same order."""
    import os
    from dgnn_amd.processing.generate_mesh import generate
    g = gold("genmesh_f4_small.npz")
    os.makedirs(os.path.join(str(tmp_path), "gt"))
    np.savez(os.path.join(str(tmp_path), "gt", "0_3dt.npz"), vertices=g["vertices"], tetrahedra=g["tetrahedra"], facets=g["facets"], nfacets=g["nfacets"])
    data = Config(path=str(tmp_path), gtfile="gt/0", filename="0", id="", category="", infinite=torch.from_numpy(g["infinite"]))
    for graph_cut in (0, 1):     # 1: gco is not installed here either -> the reference's warning and the raw labels
        clf = Config(temp=Config(graph_cut=graph_cut, fix_orientation=fix, metrics=[], device=DEV), graph_cut=Config(unary_weight=10.0, binary_weight=1.0, binary_type=0))
        mesh, ev = generate(data, torch.from_numpy(g["prediction"]).to(DEV) if graph_cut == 0 else torch.from_numpy(g["prediction"]), clf)
        assert ev == {}
        assert np.array_equal(np.asarray(mesh.faces), g["faces"]) and np.array_equal(np.asarray(mesh.vertices), g["vertices_out"])


def test_npz_ingest_matches_reference_loader_and_feeds_inference(tmp_path):
    """8f-3: dgnn_amd.processing.data.dataLoader (device fp64 standardisation) == the reference dataLoader's tensors on
    the small scene; the loaded scene then runs through inference_layer and matches the oracle on the fixture tensors."""
    import os
    from dgnn_amd.config import reconbench_pretrained
    from dgnn_amd.processing.data import dataLoader, standardize
    g = gold("ingest_small.npz")
    clf = reconbench_pretrained()
    clf.temp.cell_order = "none"          # the reference's order (file order); the relabelled scene is checked below
    dl = dataLoader(clf, verbosity=0)
    root = os.path.join(os.path.dirname(__file__), "golden", "scene_small")
    dl.run(dict(path=root, filename="0", category="", id="", scan_conf="", gtfile="gt/0", ioufile=""))
    assert dl.features.is_cuda and dl.features.dtype == torch.float32 and dl.cell_order is None
    assert dl.edge_lists.stride() == (1, 2)          # the reference's transposed view of its [E,2] array (data.py:437-438)
    assert torch.equal(dl.features[:, 0].cpu(), torch.from_numpy(g["features"][:, 0]))
    assert (dl.features.cpu() - torch.from_numpy(g["features"])).abs().max().item() <= 1e-6
    assert (dl.edge_features.cpu() - torch.from_numpy(g["edge_features"])).abs().max().item() <= 1e-6
    assert torch.equal(dl.edge_lists.cpu(), torch.from_numpy(g["edge_lists"]))
    assert torch.equal(dl.gt.cpu(), torch.from_numpy(g["gt"]))
    assert torch.equal(dl.infinite.cpu(), torch.from_numpy(g["infinite"]))
    assert dl.node_feature_names == [str(s) for s in g["node_feature_names"]]
    assert dl.getInfo() == g["features"].shape[0] and clf.temp.num_node_features == 28 and clf.temp.num_edge_features == 20
    # large-magnitude column with tiny spread: the two-pass fp64 statistics keep it exact where fp32 would not
    rng = np.random.default_rng(0)
    big = np.stack([1e3 + rng.standard_normal(5000) * 1e-3, rng.standard_normal(5000)], 1)
    ref = (big - big.mean(0)) / big.std(0)
    assert (standardize(big, 0, "cuda:0").cpu().double().numpy() - ref).__abs__().max() <= 1e-6
    # end to end from the files
    net = hip_static()
    logits = net.inference_layer(Config(x=dl.features, edge_attr=dl.edge_features, edge_index=dl.edge_lists))
    with torch.no_grad():
        want = oracle_static().inference_layer(Config(x=torch.from_numpy(g["features"]), edge_attr=torch.from_numpy(g["edge_features"]),
                                                      edge_index=torch.from_numpy(g["edge_lists"])))
    assert (logits.cpu() - want).abs().max().item() <= TOL_LOGIT * max(1.0, want.abs().max().item())
    # default: the loader relabels the cells (no _3dt.npz here -> breadth-first order of the adjacency).  Every tensor moves with its cell, the
    # graph is the same graph, and per-cell results restored to file order are the reference's
    from dgnn_amd.processing.reorder import restore_cell_order
    clf2 = reconbench_pretrained()
    d2 = dataLoader(clf2, verbosity=0)
    d2.run(dict(path=root, filename="0", category="", id="", scan_conf="", gtfile="gt/0", ioufile=""))
    co = d2.cell_order
    assert co is not None and co.kind == "bfs"
    order = co.order.cpu().long()
    n = order.numel()
    assert torch.equal(torch.sort(order).values, torch.arange(n)) and torch.equal(co.rank.cpu().long()[order], torch.arange(n))
    assert torch.equal(d2.features.cpu(), dl.features.cpu()[order]) and torch.equal(d2.gt.cpu(), dl.gt.cpu()[order])
    assert torch.equal(d2.infinite.cpu(), dl.infinite.cpu()[order])
    ei_old, ei_new = dl.edge_lists.cpu(), d2.edge_lists.cpu()
    assert torch.equal(ei_new[0], torch.arange(n).repeat_interleave(4)) and d2.edge_lists.stride() == (1, 2)
    assert torch.equal(order[ei_new[1]].view(n, 4), ei_old[1].view(-1, 4)[order])          # same neighbours, slot for slot
    assert torch.equal(d2.edge_features.cpu().view(n, 4, -1), dl.edge_features.cpu().view(-1, 4, 20)[order])
    data2 = Config(x=d2.features, edge_attr=d2.edge_features, edge_index=d2.edge_lists, infinite=d2.infinite, y=d2.gt)   # as run.py:prepareSample builds it
    logits2 = net.inference_layer(data2)
    back = restore_cell_order(logits2, data2)          # finds the order through the loader's tensors (an unmodified prepareSample)
    assert (back - logits).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item())   # same sums in another order
    assert (back.cpu() - want).abs().max().item() <= TOL_LOGIT * max(1.0, want.abs().max().item())
    assert torch.equal(restore_cell_order(d2.infinite, d2).cpu(), torch.from_numpy(g["infinite"]))
    clf2.paths = Config(out=str(tmp_path))
    d2.exportScore(logits2.cpu())
    saved = np.load(os.path.join(str(tmp_path), "prediction", "0.npz"))
    assert np.array_equal(saved["logits"], back.cpu().numpy()) and int(saved["number_of_cells"]) == n


def test_integration_md_ctypes_stub_runs_and_matches_the_oracle():
    """The ctypes stub printed in INTEGRATION.md (what a reference maintainer would paste into SAGEConv) is executed as
    is -- only the library path is made absolute -- and must reproduce the oracle's SAGEConv.forward on a bipartite block."""
    import re
    from types import SimpleNamespace
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    md = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", md, flags=re.S)
    code = next(b for b in blocks if "def forward(self, x, edge_attr, edge_index" in b)
    code = code.replace('"dgnn_amd/libdgnn_hip.so"', repr(os.path.join(root, "dgnn_amd", "libdgnn_hip.so")))
    ns = {}
    exec(compile(code, "INTEGRATION.md", "exec"), ns)
    onet = oracle_static()
    conv = onet.convs[1][0]  # 64 -> 128
    g = torch.Generator().manual_seed(9)
    n_src, n_dst, E = 900, 500, 2600
    ei = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    x = torch.randn(n_src, 64, generator=g)
    ea = torch.randn(E, 20, generator=g)
    with torch.no_grad():
        ref = conv((x, x[:n_dst]), ea, ei)
    dev_conv = SimpleNamespace(lin_e=SimpleNamespace(weight=conv.lin_e.weight.detach().to(DEV), bias=conv.lin_e.bias.detach().to(DEV)),
                               lin_j=SimpleNamespace(weight=conv.lin_j.weight.detach().to(DEV), bias=conv.lin_j.bias.detach().to(DEV),
                                                     out_features=conv.lin_j.out_features),
                               lin_i=SimpleNamespace(weight=conv.lin_i.weight.detach().to(DEV)))
    xd = x.to(DEV)
    out = ns["forward"](dev_conv, (xd, xd[:n_dst]), ea.to(DEV), ei.to(DEV))
    torch.cuda.synchronize()
    assert rel_err(out, ref.double()) < 3e-6


def test_fused_layers_chunked_over_destination_ranges_are_bit_identical():
    """Scenes beyond 2^31 activation elements are processed as consecutive destination sub-ranges; forcing the same
    mechanism on a small graph must not change a single bit (also covers a chunk boundary inside a tile)."""
    from dgnn_amd import ops
    from dgnn_amd.synthetic import delaunay_tet_graph, hashed_normal
    net = hip_static()
    adj, _, _ = delaunay_tet_graph(3000, 8)
    n = adj.shape[0] // 4
    data = Config(x=hashed_normal(np.arange(n), 29, seed=1, device=DEV), edge_attr=hashed_normal(np.arange(4 * n), 20, seed=2, device=DEV),
                  edge_index=torch.from_numpy(adj.T.astype(np.int64)).to(DEV))
    ref = net.inference_layer(data)
    old = ops.FUSED_MAX_ELEMS
    try:
        ops.FUSED_MAX_ELEMS = 128 * 3001  # ~3000 rows per launch at 128 channels, 6000+ at 64, ...
        got = net.inference_layer(data)
    finally:
        ops.FUSED_MAX_ELEMS = old
    assert torch.equal(got, ref)


def test_bn_fold_cache_follows_parameter_updates():
    """The cached BatchNorm(eval) scale/shift must be rebuilt when the statistics or affine parameters change
    (load_state_dict, an optimizer step, train-mode running statistics)."""
    g = gold("static_f2_regular256.npz")
    net = hip_static()
    data = Config(x=torch.from_numpy(g["x"]).to(DEV), edge_attr=torch.from_numpy(g["edge_attr"]).to(DEV),
                  edge_index=torch.from_numpy(g["adjacencies"].T.astype(np.int64)).to(DEV))
    a = net.inference_layer(data)
    assert np.abs(a.cpu().numpy() - g["logits"]).max() <= TOL_LOGIT
    with torch.no_grad():
        net.convs[1][1].module.running_mean.add_(0.5)      # in-place update bumps the tensor's version
    b = net.inference_layer(data)
    assert (a - b).abs().max().item() > 1e-3                 # the stale fold would have returned `a` again
    net.load_state_dict(kf96_state_dict())
    c = net.inference_layer(data)
    assert torch.equal(a, c)


def _fused_case(n_pts, c_in, c_out, seed):
    from dgnn_amd.graph import GraphPlan
    from dgnn_amd.synthetic import delaunay_tet_graph
    adj, _, _ = delaunay_tet_graph(n_pts, seed=seed)
    n = adj.shape[0] // 4
    ei = torch.from_numpy(adj.T.astype(np.int64))
    g = torch.Generator().manual_seed(seed)
    t = dict(x=torch.randn(n, c_in, generator=g), ea=torch.randn(4 * n, 20, generator=g), We=torch.randn(c_in, 20, generator=g) * 0.3,
             be=torch.randn(c_in, generator=g), Wj=torch.randn(c_out, c_in, generator=g) * 0.2, Wi=torch.randn(c_out, c_in, generator=g) * 0.2,
             bj=torch.randn(c_out, generator=g))
    return n, ei, GraphPlan(ei.to(DEV), n, n), t


def _fused_run(plan, n, t, mode):
    from dgnn_amd import ops
    d = {k: v.to(DEV) for k, v in t.items()}
    return ops.sage_layer_fused_fwd(plan.rowptr, plan.src, n, d["x"], d["ea"], d["We"], d["be"], d["Wj"], d["bj"], d["Wi"], None, None, False,
                                    gemm_mode=mode, eid=plan.eid).cpu().double()


def _fused_ref(n, ei, t):
    from oracle.pyg_semantics import propagate_mean
    phi = t["ea"].double() @ t["We"].double().t() + t["be"].double()
    a = propagate_mean(t["x"].double(), n, ei, phi)
    return a @ t["Wj"].double().t() + t["bj"].double() + t["x"].double() @ t["Wi"].double().t()


@pytest.mark.parametrize("c_in,c_out", [(28, 64), (64, 128), (128, 128)])
def test_f16x2_group_scales_cover_the_fp32_range(c_in, c_out):
    """The fp16 two-part form scales every operand group by a power of two first (fp16 has 5 exponent bits).  Rows, attribute blocks and weight
    matrices spread over 60 binades must come out as accurately, row by row, as in the bf16 x 3 form (which needs no scaling)."""
    from dgnn_amd import ops
    n, ei, plan, t = _fused_case(900, c_in, c_out, seed=c_in + 1)
    g = torch.Generator().manual_seed(5)
    # every cell's feature row and every edge's attribute row gets its own magnitude, 2^-30 .. 2^30; the weights sit at 1e-6 and 1e+4
    t["x"] = t["x"] * torch.exp2(torch.randint(-30, 31, (n, 1), generator=g).float())
    t["ea"] = t["ea"] * torch.exp2(torch.randint(-30, 31, (4 * n, 1), generator=g).float())
    t["Wj"], t["Wi"], t["We"] = t["Wj"] * 1e-6, t["Wi"] * 1e-6, t["We"] * 1e4
    ref = _fused_ref(n, ei, t)
    # error of a row relative to the magnitude of the terms that make it up (its own row and its neighbours' messages differ by up to 2^60)
    phi = (t["ea"].double() @ t["We"].double().t() + t["be"].double()).abs()
    from oracle.pyg_semantics import propagate_mean
    mag = propagate_mean(t["x"].double().abs(), n, ei, phi) @ t["Wj"].double().abs().t() + t["x"].double().abs() @ t["Wi"].double().abs().t() + t["bj"].double().abs()
    errs = {}
    for mode in (ops.GEMM_BF16X3_FILTER, ops.GEMM_F16X2):
        out = _fused_run(plan, n, t, mode)
        assert torch.isfinite(out).all()
        errs[mode] = ((out - ref).abs() / mag).max().item()
    print("rows over 60 binades, %d->%d: max err / sum|terms|  bf16x3 %.2e  f16x2 %.2e" % (c_in, c_out, errs[ops.GEMM_BF16X3_FILTER], errs[ops.GEMM_F16X2]))
    assert errs[ops.GEMM_F16X2] < 1e-6 and errs[ops.GEMM_F16X2] < 4 * errs[ops.GEMM_BF16X3_FILTER] + 1e-7, errs


def test_f16x2_zero_rows_tiny_rows_and_nan_stay_local():
    from dgnn_amd import ops
    n, ei, plan, t = _fused_case(700, 128, 128, seed=3)
    t["x"][5] = 0.0                       # an all-zero cell
    t["x"][6] = 1e-38                     # a cell at the bottom of the fp32 range
    t["x"][7] = 1e30                      # and one near the top (its products with the weights stay below the fp32 maximum)
    t["ea"][40:44] = 0.0                  # a cell whose in-edges carry no attributes
    ref = _fused_ref(n, ei, t)
    out = _fused_run(plan, n, t, ops.GEMM_F16X2)
    finite = torch.isfinite(ref).all(1)
    assert torch.isfinite(out[finite]).all()
    scale = ref[finite].abs().max(1, keepdim=True).values.clamp_min(1.0)
    assert ((out[finite] - ref[finite]).abs() / scale).max().item() < 2e-6
    # a NaN feature row poisons its own output row and those of the cells that aggregate it -- nothing else
    t["x"][100, 3] = float("nan")
    out = _fused_run(plan, n, t, ops.GEMM_F16X2)
    touched = torch.zeros(n, dtype=torch.bool)
    touched[100] = True
    touched[ei[1][ei[0] == 100]] = True
    assert torch.isnan(out[touched]).any(1).all()
    assert torch.isfinite(out[~touched & finite]).all()


@pytest.mark.parametrize("k1,k2,n_out", [(256, 256, 512), (128, 128, 256), (100, 0, 200), (512, 512, 1024)])
def test_linear_fwd_x2h_vs_fp64(k1, k2, n_out):
    """The wide layers' GEMM in the fp16 two-part form (row scales, 3 products) against fp64 and against the bf16 x 3 form: rows of A over
    40 binades, weight rows over 20, BatchNorm / ReLU epilogue, a ragged last tile."""
    from dgnn_amd import ops
    M = 8192 + 77
    g = torch.Generator().manual_seed(k1 + n_out)
    A1 = torch.randn(M, k1, generator=g) * torch.exp2(torch.randint(-20, 21, (M, 1), generator=g).float())
    W1 = torch.randn(n_out, k1, generator=g) * 0.1 * torch.exp2(torch.randint(-10, 11, (n_out, 1), generator=g).float())
    A2 = torch.randn(M, k2, generator=g) * A1.abs().max(1, keepdim=True).values * 0.5 if k2 else None
    W2 = torch.randn(n_out, k2, generator=g) * 0.1 if k2 else None
    b, sc, sh = torch.randn(n_out, generator=g), torch.rand(n_out, generator=g) + 0.5, torch.randn(n_out, generator=g)
    z = A1.double() @ W1.double().t() + (A2.double() @ W2.double().t() if k2 else 0.0) + b.double()
    ref = torch.relu(z * sc.double() + sh.double())
    mag = (A1.double().abs() @ W1.double().abs().t() + (A2.double().abs() @ W2.double().abs().t() if k2 else 0.0) + b.double().abs()) * sc.double() + sh.double().abs()
    dev = lambda t: None if t is None else t.to(DEV)
    errs, old = {}, ops.GEMM_MODE
    try:
        for mode in (ops.GEMM_BF16X3_FILTER, ops.GEMM_F16X2):
            ops.GEMM_MODE = mode
            out = ops.linear_fwd(dev(A1), dev(W1), dev(A2), dev(W2), dev(b), dev(sc), dev(sh), True).cpu().double()
            errs[mode] = ((out - ref).abs() / mag).max().item()
    finally:
        ops.GEMM_MODE = old
    print("x2h GEMM K=%d+%d N=%d: max err / sum|terms|  x3 %.2e  x2h %.2e" % (k1, k2, n_out, errs[ops.GEMM_BF16X3_FILTER], errs[ops.GEMM_F16X2]))
    assert errs[ops.GEMM_F16X2] < 1e-6 and errs[ops.GEMM_F16X2] < 4 * errs[ops.GEMM_BF16X3_FILTER] + 1e-7, errs
    if n_out > 256:
        # operands split once by their own pass + DMA staging (x2hp, opt-in DGNN_X2HP=1) == split inside the GEMM's K loop (x2h): bit for bit
        outs = []
        old_hp = ops.X2HP
        try:
            for hp in (True, False):
                ops.X2HP = hp
                outs.append(ops.linear_fwd(dev(A1), dev(W1), dev(A2), dev(W2), dev(b), dev(sc), dev(sh), True))
        finally:
            ops.X2HP = old_hp
        assert torch.equal(outs[0], outs[1]) and (outs[0].cpu().double() - ref).abs().max().item() > 0      # (and it is the fp16 two-part arithmetic, not fp64)


def test_plan_grouped_trusted_hint_is_the_grouped_plan_in_one_launch():
    """DGNN_PLAN_HINT_GROUPED_TRUSTED (ring parts: the list was laid out grouped by destination by this package): the same plan as the verified GROUPED builder,
    with rows without edges at the start / middle / end; a list that breaks the promise gives some plan inside its arrays (no fault), an empty list works"""
    from dgnn_amd import ops
    rng = np.random.default_rng(3)
    n_dst, n_src = 4000, 6000
    deg = rng.integers(0, 7, n_dst)
    deg[:5] = 0; deg[2000:2010] = 0; deg[-7:] = 0
    dst = np.repeat(np.arange(n_dst), deg)
    ei = torch.from_numpy(np.stack([rng.integers(0, n_src, dst.shape[0]), dst])).to(DEV)
    want = ops.plan_build(ei, n_dst, by=1, hint=ops.PLAN_HINT_GROUPED, n_other=n_src)
    got = ops.plan_build(ei, n_dst, by=1, hint=ops.PLAN_HINT_GROUPED_TRUSTED, n_other=n_src)
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    bad = ei.clone()
    bad[1] = bad[1].flip(0)                                # descending keys: the promise is broken
    bad[1, 17] = n_dst + 12345                             # ... and one key out of range
    rp, oth, eid = ops.plan_build(bad, n_dst, by=1, hint=ops.PLAN_HINT_GROUPED_TRUSTED, n_other=n_src)
    torch.cuda.synchronize()
    assert rp.numel() == n_dst + 1 and int(rp.max()) <= bad.size(1) and int(oth.max()) < n_src
    rp0, _, _ = ops.plan_build(torch.zeros(2, 0, dtype=torch.int64, device=DEV), 5, by=1, hint=ops.PLAN_HINT_GROUPED_TRUSTED)
    assert torch.equal(rp0.cpu(), torch.zeros(6, dtype=torch.int32))
