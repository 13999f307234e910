"""GPU parity at the sizes that are benchmarked: the 1 010 078-tet metric graph against the fp32
oracle evaluated on the host cores of the GPU box, the WHOLE real Ignatius scene against logits produced by the
reference's own model file (tests/golden/static_f4_ignatius_full.npz), and the layer-major schedule against the
reference's own inference_layer_batch output (static_f5_layer_batch.npz).

Tolerance (stated): |dlogit| <= 1e-4 * max(1, |logit|).  On synthetic N(0,1) inputs logits stay within +-8 and this is the
1e-4 absolute bound of SURVEY 8c; on the real scene standardised features reach 174 sigma, logits +-167, and the
reference's fp32 result itself sits 5.3e-5 (1e-5 relative) away from its fp64 evaluation -- an absolute 1e-4 would be
tighter than the reference is with itself.  Next to it the fp64 yardstick: the HIP logits may be at most 3x as far from
the reference's fp64 evaluation as the reference's own fp32 logits are."""
import os

import numpy as np
import pytest
import torch

from dgnn_amd.config import Config
from helpers import gold, oracle_static
from test_gpu_parity import DEV, TOL_LOGIT, hip_static

pytestmark = pytest.mark.gpu


def logit_check(got, ref, ref64=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = TOL_LOGIT * np.maximum(1.0, np.abs(ref))
    err = np.abs(got - ref)
    assert (err <= tol).all(), "max|dlogit| %.3e (tol %.1e at that entry)" % (err.max(), tol.reshape(-1)[err.argmax()])
    margin = np.abs(ref[:, 0] - ref[:, 1]) > 2 * tol.max(axis=1)
    flips = int((got.argmax(1)[margin] != ref.argmax(1)[margin]).sum())
    assert flips == 0, "%d arg-max flips among %d cells with a margin above the tolerance" % (flips, int(margin.sum()))
    if ref64 is not None:
        e_ref, e_got = np.abs(ref - ref64).max(), np.abs(got - ref64).max()
        assert e_got <= max(3 * e_ref, 1e-5), "error vs fp64: ours %.3e, the reference's own %.3e" % (e_got, e_ref)
    return float(err.max())


def assert_grads_within_rounding_model(mgrads, hgrads, rms_bound=1e-3, outside_per=1000, cap=2e-2, line_bound=None, zero_keys=(), zero_floor=5e-6):
    """The structured bound on HIP parameter gradients against a storage-rounding model (tests/bf16_training_model.py), per tensor:
    rms of the difference <= rms_bound of the tensor's rms; at most one in `outside_per` of the entries (two for a bias vector) beyond fp32 class
    (1e-3 of the tensor's largest entry), and those shaped like flipped mask entries (row-shaped, see below) -- outside_per None: no such count,
    for differences that are dense by nature; every entry within `cap` of the tensor's largest; line_bound: the rms of the difference along any
    single row or column <= line_bound of the tensor's rms (a mis-indexed channel is a whole wrong row or column).  zero_keys: tensors with an
    analytically zero gradient (biases ahead of a train-mode BatchNorm), which hold rounding noise on both sides: 5e-4 of their own largest entry
    plus `zero_floor` of the largest gradient in the model (the fp32 tests' 5e-6 by default)."""
    from bf16_training_model import error_table
    vs_model = error_table(mgrads, hgrads)
    mmax = max(g.abs().max().item() for g in mgrads.values())
    for k, (mx, rms) in vs_model.items():
        ref_k = mgrads[k]
        d = (hgrads[k].double().cpu() - ref_k).abs()
        top_k = ref_k.abs().max().item()
        if k in zero_keys:
            assert d.max().item() <= 5e-4 * top_k + zero_floor * mmax, (k, d.max().item(), top_k, mmax)
            continue
        assert rms <= rms_bound and d.max().item() <= cap * top_k + 1e-6 * mmax, (k, mx, rms)
        if line_bound is not None and d.dim() == 2:
            rr = ref_k.pow(2).mean().sqrt().item()
            line = max(d.pow(2).mean(dim=1).sqrt().max().item(), d.pow(2).mean(dim=0).sqrt().max().item())
            assert line <= line_bound * rr, (k, line / rr)
        if outside_per is None:
            continue
        far = d > 1e-3 * top_k + 1e-6 * mmax
        outside = int(far.sum().item())       # entries beyond fp32 class: at most 0.1 % of the tensor (two for a bias vector)
        assert outside <= max(2, d.numel() // outside_per), (k, mx, rms, outside, d.numel())
        # ... and they have the SHAPE of a flipped mask entry: a flip at (cell, channel j) changes dz[cell, j] alone, i.e. ROW j of the layer's dWl / dWr
        # (by delta * a[cell, :] resp. delta * x[cell, :]: part of that row crosses the fp32 class, measured up to 38 of 256 entries) and nothing of any
        # other row.  So: at most max(2, 1 %) of a weight gradient's rows may hold more than 2 % of their entries outside, and none more than a quarter
        # -- a mis-indexed channel (a whole wrong row or column) cannot hide in the 0.1 % allowance above.
        if d.dim() == 2 and d.size(1) >= 16:
            per_row, per_col = far.sum(dim=1), far.sum(dim=0)
            rows_hit = int((per_row > max(2, d.size(1) // 50)).sum().item())
            assert rows_hit <= max(2, d.size(0) // 100) and int(per_row.max().item()) <= max(4, d.size(1) // 4) and int(per_col.max().item()) <= max(4, d.size(0) // 4), \
                (k, rows_hit, int(per_row.max().item()), int(per_col.max().item()), tuple(d.shape))


_scene = {}


def metric_graph():
    """The BASELINE.md metric graph (bench.py's generator and seeds), built once per test session."""
    if not _scene:
        import bench
        adj, _, x, ea = bench.make_scene(150000, 0)
        _scene.update(adj=adj, x=x, ea=ea, ei=torch.from_numpy(adj.T.astype(np.int64)))
    return _scene


def test_metric_graph_1m_vs_oracle_all_gemm_modes():
    """N = 1 010 078, E = 4 040 312: inference_layer in all three matrix-core modes against the fp32 oracle on the host CPU;
    per-layer relu0..3 on a 50k-row sample against the oracle's trace."""
    from dgnn_amd import ops
    from dgnn_amd.graph import GraphPlan
    s = metric_graph()
    n = s["x"].shape[0]
    assert n == 1010078
    onet = oracle_static()
    trace = []
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    with torch.no_grad():
        ref = onet.inference_layer(Config(x=s["x"], edge_attr=s["ea"], edge_index=s["ei"]), trace)
    ref = ref.numpy()
    rows = torch.arange(0, n, 20)
    tr = {k: v[rows].clone() for k, v in trace if k.startswith("relu")}
    tr_all = {k: v for k, v in trace if k.startswith("relu")}   # every row, for the default mode (a rare single-row fault must not slip through a stride)
    del trace
    net = hip_static()
    data = Config(x=s["x"].to(DEV), edge_attr=s["ea"].to(DEV), edge_index=s["ei"].to(DEV))
    old = ops.GEMM_MODE
    try:
        for mode in (ops.GEMM_F16X2, ops.GEMM_F16X2_DENSE, ops.GEMM_BF16X3_FILTER, ops.GEMM_BF16X3, ops.GEMM_F32):
            ops.GEMM_MODE = mode
            logits = net.inference_layer(data).cpu().numpy()
            err = logit_check(logits, ref)
            print("mode %d: max|dlogit| %.3e over %d tets" % (mode, err, n))
            assert err <= 1e-4        # SURVEY 8c's FLAT bound on the metric graph (logits within +-8): holds with a 10x margin in every mode
            # layer trace: each fused layer on the device, 50k sampled rows against the oracle's activations
            plan = GraphPlan(data.edge_index, n, n, hint=ops.PLAN_HINT_REFERENCE)
            h = data.x[:, 1:]
            for i in range(4):
                h = net._eval_layers(h, n, data.edge_attr, [plan] * 4, True, only=i)
                got, want = h[rows.to(DEV)].cpu().double(), tr["relu%d" % i].double()
                rel = ((got - want).abs().max() / want.abs().max()).item()
                assert rel < 2e-5, (mode, i, rel)
                if mode == ops.GEMM_F16X2:      # the default arithmetic: ALL 1 010 078 rows of every layer against the oracle's trace
                    want_d = tr_all["relu%d" % i].to(DEV)
                    bad = ((h - want_d).abs() > 2e-5 * want_d.abs().max()).any(1).nonzero().flatten()
                    assert bad.numel() == 0, (i, bad[:8].tolist())
                    del want_d
    finally:
        ops.GEMM_MODE = old


def test_metric_graph_1m_properties():
    """Size-independent properties at full size: bit-identical repeat runs, a plan built by the generic kernels gives the
    same logits as the verified fast path, and relabelling the cells (a permutation of the graph) permutes the logits."""
    from dgnn_amd import ops
    from dgnn_amd.graph import GraphPlan
    s = metric_graph()
    n = s["x"].shape[0]
    net = hip_static()
    data = Config(x=s["x"].to(DEV), edge_attr=s["ea"].to(DEV), edge_index=s["ei"].to(DEV))
    a = net.inference_layer(data)
    b = net.inference_layer(data)
    assert torch.equal(a, b)
    g = net.inference_layer(data, plan=GraphPlan(data.edge_index, n, n, hint=ops.PLAN_HINT_GENERIC))
    assert torch.equal(a, g)
    # relabel: new id = perm[old id]; rows of x move with their cell, edge rows stay attached to their (src,dst) pair.
    # Each destination still sums its 4 messages, in a different order -> equal up to fp32 summation order.
    gen = torch.Generator().manual_seed(3)
    perm = torch.randperm(n, generator=gen)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    ei_p = perm[s["ei"]]                     # same edge positions, relabelled endpoints (no longer the reference layout)
    data_p = Config(x=s["x"][inv].to(DEV), edge_attr=data.edge_attr, edge_index=ei_p.to(DEV))
    c = net.inference_layer(data_p)          # generic plan builder (the fast paths reject this layout on the device)
    d = (c[perm.to(DEV)] - a).abs().max().item()
    assert d <= 2e-5, d


def test_ignatius_full_scene_vs_reference_logits():
    """67 017 cells in CGAL order (neighbour ids tens of thousands of rows apart), real standardised features; expected
    logits come from the reference's own surfaceNetStaticEdgeFilters.inference_layer (make_golden.py ignatius_full)."""
    from dgnn_amd import ops
    g = gold("static_f4_ignatius_full.npz")
    n = g["x"].shape[0]
    fg = np.random.default_rng(int(g["fgeom_seed"])).standard_normal((4 * n, 4)).astype(np.float32)
    ea = np.concatenate([fg, g["edge_attr16"]], axis=1)
    adj = np.stack([np.repeat(np.arange(n, dtype=np.int64), 4), g["adj_dst"].astype(np.int64)])
    data = Config(x=torch.from_numpy(g["x"]).to(DEV), edge_attr=torch.from_numpy(ea).to(DEV), edge_index=torch.from_numpy(adj).to(DEV))
    net = hip_static()
    old = ops.GEMM_MODE
    try:
        for mode in (ops.GEMM_F16X2, ops.GEMM_F16X2_DENSE, ops.GEMM_BF16X3_FILTER, ops.GEMM_BF16X3, ops.GEMM_F32):
            ops.GEMM_MODE = mode
            logits = net.inference_layer(data).cpu().numpy()
            err = logit_check(logits, g["logits"], g["logits64"])
            print("Ignatius mode %d: max|dlogit| %.3e (logit range %.0f)" % (mode, err, np.abs(g["logits"]).max()))
    finally:
        ops.GEMM_MODE = old
    # layer trace on the stored row sample
    from dgnn_amd.graph import GraphPlan
    plan = GraphPlan(data.edge_index, n, n, hint=ops.PLAN_HINT_REFERENCE)
    rows = torch.from_numpy(g["trace_rows"]).to(DEV)
    h = data.x.contiguous()[:, 1:]          # the fixture keeps the loader's column-major layout (pandas -> torch)
    for i in range(4):
        h = net._eval_layers(h, n, data.edge_attr, [plan] * 4, True, only=i)
        want = torch.from_numpy(g["relu%d_rows" % i]).double()
        rel = ((h[rows].cpu().double() - want).abs().max() / want.abs().max()).item()
        assert rel < 2e-5, (i, rel)
    # the unfused aggregate + GEMM pair on the same scene (what other widths and training use)
    ops.FUSED_ENABLED = False
    try:
        logit_check(net.inference_layer(data).cpu().numpy(), g["logits"], g["logits64"])
    finally:
        ops.FUSED_ENABLED = True


def test_layer_batch_vs_reference_and_oracle():
    """inference_layer_batch (layer-major, 1-hop blocks): against the reference's own output on the same blocks and
    against the oracle's inference_layer_batch -- not against another HIP path."""
    from oracle.pyg_semantics import neighbor_sampler_full
    g = gold("static_f5_layer_batch.npz")
    adj = g["adjacencies"]
    n = adj.shape[0] // 4
    ei = adj.T.astype(np.int64)
    bs = int(g["batch_size"])
    loader = []
    for s in range(0, n, bs):
        b = np.arange(s, min(n, s + bs))
        n_id, adjs = neighbor_sampler_full(ei, n, b, 1)
        a, e, size = adjs[0]
        loader.append((len(b), torch.from_numpy(n_id), (torch.from_numpy(a), torch.from_numpy(e), size)))
    x, ea = torch.from_numpy(g["x"]), torch.from_numpy(g["edge_attr"])
    net = hip_static()
    got = net.inference_layer_batch(Config(x=x.to(DEV), edge_attr=ea.to(DEV)), loader).cpu().numpy()
    logit_check(got, g["logits"])
    with torch.no_grad():
        oref = oracle_static().inference_layer_batch(Config(x=x, edge_attr=ea), loader).numpy()
    logit_check(got, oref)
    # the GPU block builder as the loader (what a reference run.py would construct, run.py:221-223)
    from dgnn_amd.sampler import NeighborSampler
    gl = NeighborSampler(torch.from_numpy(ei).to(DEV), sizes=[-1], num_nodes=n, batch_size=bs, shuffle=False)
    got2 = net.inference_layer_batch(Config(x=x.to(DEV), edge_attr=ea.to(DEV)), gl).cpu().numpy()
    logit_check(got2, g["logits"])


def test_out_of_range_edge_index_is_reported_not_corrupting():
    """A malformed adjacency (-1 neighbours, ids >= N) must not write outside the plan arrays; the error surfaces at a later
    call as DGNN_E_INDEX (torch's scatter raises an index error in the reference)."""
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    n = 1000
    gen = torch.Generator().manual_seed(0)
    ei = torch.randint(0, n, (2, 4000), generator=gen)
    bad = ei.clone()
    bad[1, 17] = -1
    bad[1, 99] = n + 5
    bad[0, 5] = n  # source out of range
    guard = torch.full((8192,), 12345, dtype=torch.int32, device=DEV)  # canary allocations around the plan
    with pytest.raises(DgnnError, match="out of range"):
        rowptr, src, eid = ops.plan_build(bad.to(DEV), n, by=1, hint=ops.PLAN_HINT_GENERIC, n_other=n)
        torch.cuda.synchronize()
        assert int(rowptr[-1]) == 4000 - 2           # the two bad-key edges are left out
        assert int(src.max()) < n and int(src[: int(rowptr[-1])].min()) >= 0
        ops.plan_build(ei.to(DEV), n, by=1, n_other=n)   # the next index-consuming entry point (or any 16th call) reports it
    assert bool((guard == 12345).all())
    # the report is asynchronous: kernels that were still running when it was raised may add to it; drain it after a sync
    from dgnn_amd._lib import lib
    torch.cuda.synchronize()
    lib().dgnn_poll_async_error()
    # and the flag is cleared: a good plan afterwards works
    rowptr, src, eid = ops.plan_build(ei.to(DEV), n, by=1, n_other=n)
    torch.cuda.synchronize()
    ops.relu(torch.zeros(4, device=DEV))
    assert int(rowptr[-1]) == 4000


def test_fused_predicate_matches_dispatch_128_to_64():
    """convs [..,128,64] must fall back to the aggregate + GEMM pair instead of raising."""
    from dgnn_amd.synthetic import delaunay_tet_graph
    adj, _, _ = delaunay_tet_graph(800, seed=2)
    n = adj.shape[0] // 4
    gen = torch.Generator().manual_seed(1)
    x, ea = torch.randn(n, 29, generator=gen), torch.randn(4 * n, 20, generator=gen)
    ei = torch.from_numpy(adj.T.astype(np.int64))
    convs = (64, 128, 64, 100)
    onet = oracle_static(convs=convs, load=False, seed=4)
    net = hip_static(convs=convs, sd=onet.state_dict())
    with torch.no_grad():
        ref = onet.inference_layer(Config(x=x, edge_attr=ea, edge_index=ei)).numpy()
    got = net.inference_layer(Config(x=x.to(DEV), edge_attr=ea.to(DEV), edge_index=ei.to(DEV))).cpu().numpy()
    logit_check(got, ref)


def reached(entry, expect, M, n_out, K):
    """the kernel the last dense forward call of this thread chose (dgnn_debug_last_linear_variant) is `expect` -- what these tests used to trust
    a comment for.  `expect` holds under the default switches; with a switch set, the mirrored dispatch of tests/gemm_model.py decides."""
    import gemm_model as gm
    from dgnn_amd._lib import lib
    on = gm.env_switches()
    got = gm.VARIANT_NAMES[lib().dgnn_debug_last_linear_variant()]
    assert got == gm.expected_variant(entry, M, n_out, K, on), (got, M, n_out, K)
    if all(on.values()):
        assert got == expect, (got, expect, M, n_out, K)


@pytest.mark.parametrize("k1,k2,n_out", [(256, 256, 512), (128, 128, 256), (70, 0, 300), (512, 512, 1024)])
def test_x3_gemm_large_tile_equals_the_small_tile_and_fp64(monkeypatch, k1, k2, n_out):
    """dgnn_linear_fwd_x3 takes a 256 x 256 tile for M >= 8192, n_out > 128: per output element the same chunk and product
    order as the 128 x 128 tile (reached here by calling it on row slices below the threshold), so results are bit-identical;
    and both are fp32-class against an fp64 product.
    What the dispatch observer shows (`whole`, `slices`, `last` below: the kernels of the whole call, the 4096-row slices and the ragged last
    slice): since the 256 x 256 tile asks for 192 tiles, NONE of these shapes reaches it any more (35 row blocks x 1..4 column blocks) -- they
    compare the 128 x 128, 64 x 64 and small-problem kernels with each other.  k_linear_fwd_x3_big is held to fp64 in test_gpu_gemm_edges.py."""
    whole, slices, last = {512: ("X3", "X3_MID1", "X3_SMALL"), 256: ("X3_SMALL",) * 3, 300: ("X3_SMALL",) * 3, 1024: ("X3", "X3", "X3_MID4")}[n_out]
    from dgnn_amd import ops
    monkeypatch.setattr(ops, "GEMM_MODE", ops.GEMM_BF16X3)
    g = torch.Generator().manual_seed(k1 + n_out)
    M = 8192 + 2 * 256 + 77                                # ragged last row block
    A1 = torch.randn(M, k1, generator=g).to(DEV)
    W1 = (torch.randn(n_out, k1, generator=g) / k1 ** 0.5).to(DEV)
    A2 = torch.randn(M, k2, generator=g).to(DEV) if k2 else None
    W2 = (torch.randn(n_out, k2, generator=g) / k2 ** 0.5).to(DEV) if k2 else None
    bias = torch.randn(n_out, generator=g).to(DEV)
    big = ops.linear_fwd(A1, W1, A2, W2, bias, relu=True)
    reached("x3", whole, M, n_out, k1 + k2)
    parts = []
    for s in range(0, M, 4096):
        parts.append(ops.linear_fwd(A1[s:s + 4096], W1, A2[s:s + 4096] if k2 else None, W2, bias, relu=True))
        reached("x3", slices if s + 4096 <= M else last, min(4096, M - s), n_out, k1 + k2)
    small = torch.cat(parts)
    ref = A1.double() @ W1.double().t() + bias.double()
    if k2:
        ref = ref + A2.double() @ W2.double().t()
    ref = ref.clamp_min(0)
    if k1 + k2 >= 1024:
        # round 6: the ragged last slice (589 rows, K = 1024) takes the 64 x 64 tiles with four K groups per workgroup (k_linear_fwd_x3_mid<4>):
        # another summation order, fp32 rounding level; the 4096-row slices take the 128 x 128 tiles: the same bits as the large tile
        assert torch.equal(big[:8192], small[:8192])
        assert (big.double() - small.double()).abs().max().item() <= 2e-6 * ref.abs().max().item()
    else:
        assert torch.equal(big, small)
    assert (big.double() - ref).abs().max().item() <= 4e-6 * ref.abs().max().item()
    assert (small.double() - ref).abs().max().item() <= 4e-6 * ref.abs().max().item()


@pytest.mark.parametrize("k1,k2,n_out", [(28, 28, 64), (128, 0, 64), (64, 64, 28), (64, 0, 2), (512, 0, 64), (70, 33, 37)])
def test_x3_gemm_narrow_tile_equals_the_128_wide_tile(monkeypatch, k1, k2, n_out):
    """n_out <= 64 takes a 128 x 64 tile; per output element it is the 128 x 128 kernel's arithmetic (reached here by padding W with zero
    rows to 128 outputs), so the shared columns are bit-identical.
    What the dispatch observer shows: at M = 5077 (below the small-problem threshold of 16384 rows) the narrow call takes the small-problem
    kernel and the padded one that or, at K = 512, the 64 x 64 tiles -- neither k_linear_fwd_x3_n64 nor the 128 x 128 tile.  The comparison
    still holds between the kernels it reaches; the narrow and the 128 x 128 tile are held to fp64 in test_gpu_gemm_edges.py."""
    from dgnn_amd import ops
    monkeypatch.setattr(ops, "GEMM_MODE", ops.GEMM_BF16X3)
    g = torch.Generator().manual_seed(k1 * 7 + n_out)
    M = 5000 + 77
    A1 = torch.randn(M, k1, generator=g).to(DEV)
    W1 = (torch.randn(n_out, k1, generator=g) / k1 ** 0.5).to(DEV)
    A2 = torch.randn(M, k2, generator=g).to(DEV) if k2 else None
    W2 = (torch.randn(n_out, k2, generator=g) / k2 ** 0.5).to(DEV) if k2 else None
    bias = torch.randn(n_out, generator=g).to(DEV)
    pad = lambda W: torch.cat([W, torch.zeros(128 - n_out, W.size(1), device=DEV)])
    narrow = ops.linear_fwd(A1, W1, A2, W2, bias, relu=True)
    reached("x3", "X3_SMALL", M, n_out, k1 + k2)
    wide = ops.linear_fwd(A1, pad(W1), A2, pad(W2) if k2 else None, torch.cat([bias, torch.zeros(128 - n_out, device=DEV)]), relu=True)
    reached("x3", "X3_MID1" if k1 + k2 >= 512 else "X3_SMALL", M, 128, k1 + k2)
    assert torch.equal(narrow, wide[:, :n_out])
    acc = torch.randn(M, n_out, generator=g).to(DEV)      # the accumulate flag of the backward pass
    out = acc.clone()
    from dgnn_amd._lib import lib, ptr, stream_ptr, check
    check(lib().dgnn_linear_fwd_x3(ptr(A1), A1.stride(0), k1, ptr(W1), k1, None, 0, 0, None, 0, None, None, None, 2, M, n_out, ptr(out), n_out, stream_ptr()), "x3")
    ref = acc + ops.linear_fwd(A1, W1)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("convs,points,batch", [((64, 128, 128, 128), 150000, 2048), ((64, 128, 256, 512), 30000, 1024), ((128, 256, 512, 1024), 30000, 1024)])
def test_training_step_at_bench_scale_matches_the_oracle(convs, points, batch):
    """One training step on a 2048-target 4-hop block of the bench scene (~138k cells, the size tools/bench_train.py times): block built
    by the GPU block builder, forward in train mode + the Trainer's loss + backward through the composite HIP entry points, against the
    CPU oracle (fp64) on the same block: logits, loss, every parameter gradient and the BatchNorm running buffers.
    Round 4: also at the widths the reference TRAINS with -- [64,128,256,512] (configs/eth.yaml:56, aerial.yaml:57, terrestrial.yaml:56) and
    [128,256,512,1024] at batch 1024 (configs/modelnet.yaml:44,56, shapenet.yaml:56) -- random-init weights, a 200k-tet scene."""
    from dgnn_amd.learning.runModel import Metrics, Trainer
    from dgnn_amd.sampler import NeighborSampler
    from helpers import kf96_state_dict, oracle_static
    from test_trainer_cpu import make_clf
    from dgnn_amd.synthetic import delaunay_tet_graph, hashed_normal
    shipped = tuple(convs) == (64, 128, 128, 128)
    adj, _, _ = delaunay_tet_graph(points, 0)
    n = adj.shape[0] // 4
    ei = torch.from_numpy(adj.T.astype(np.int64)).to(DEV)
    x = hashed_normal(np.arange(n), 29, seed=1, device=DEV)
    x[:, 0] = x[:, 0].abs() + 0.05
    ea = hashed_normal(np.arange(4 * n), 20, seed=2, device=DEV)
    occ = torch.sigmoid(2 * x[:, 3:4] + x[:, 7:8])
    y = torch.cat([occ, 1 - occ], 1)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:batch].to(DEV)
    _, n_id, adjs = NeighborSampler(ei, sizes=[-1] * 4, num_nodes=n, batch_size=batch).sample(idx)
    assert n_id.numel() > (100000 if shipped else 40000)
    # HIP
    clf = make_clf()
    clf.model.convs = list(convs)
    clf.temp.device = DEV
    clf.training.metrics = Metrics()
    from test_gpu_parity import hip_static
    sd0 = None if shipped else oracle_static(convs=convs, load=False, seed=11).state_dict()
    net = hip_static(train=True, convs=convs, sd=sd0)
    tr = Trainer(net)
    data = Config(all=Config(x=x, y=y, edge_attr=ea), batch_n_id=n_id, batch_adjs=adjs)
    logits = net(data)
    ids = n_id[:batch]
    data.batch_x, data.batch_gt = x[ids], y[ids]
    loss = tr.calcLossAndOA(logits, None, data, clf, clf.training.metrics)
    loss.backward()
    # oracle, fp64 on the CPU, same block
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    onet = oracle_static(train=True, dtype=torch.float64, convs=convs, load=shipped, seed=11)
    cdata = Config(all=Config(x=x.double().cpu(), edge_attr=ea.double().cpu()), batch_n_id=n_id.cpu(),
                   batch_adjs=[(a.cpu(), e.cpu(), s) for a, e, s in adjs])
    ologits = onet(cdata)
    import torch.nn.functional as F
    gt, w = y[ids].double().cpu(), x[ids, 0].double().cpu()
    cell = F.kl_div(F.log_softmax(ologits, dim=-1), gt, reduction="none").sum(1) * w
    oloss = cell.sum() / w.sum()
    oloss.backward()
    assert (logits.detach().double().cpu() - ologits.detach()).abs().max().item() <= 2e-4 * max(1.0, ologits.abs().max().item())
    assert abs(loss.item() - oloss.item()) <= 2e-5 * abs(oloss.item()) + 1e-9
    ograds = {k: p.grad for k, p in onet.named_parameters()}
    gmax = max(g.abs().max().item() for g in ograds.values())
    for k, p in net.named_parameters():
        err = (p.grad.double().cpu() - ograds[k]).abs().max().item()
        assert err <= 5e-4 * ograds[k].abs().max().item() + 5e-6 * gmax, (k, err, ograds[k].abs().max().item(), gmax)
    ob = dict(onet.named_buffers())
    for k, b in net.named_buffers():
        ref = ob[k].double()
        assert (b.double().cpu() - ref).abs().max().item() <= 1e-5 * max(ref.abs().max().item(), 1e-30) + 1e-12, k
    assert clf.training.metrics.samples_sum == batch


@pytest.mark.parametrize("dtype,params,points,batch", [(torch.float32, (64, 128, 128, 128), 30000, 2048), (torch.bfloat16, (64, 128, 128, 128), 30000, 2048),
                                                       (torch.bfloat16, (64, 128, 256, 512), 10000, 1024), (torch.float32, (64, 128, 256, 512), 10000, 1024),
                                                       (torch.bfloat16, (128, 256, 512, 1024), 10000, 1024), (torch.float32, (128, 256, 512, 1024), 10000, 1024)])
def test_updated_training_step_at_scale_matches_the_oracle(dtype, params, points, batch):
    """Updated variant ("sage": the reference's "sage+" head cannot be differentiated -- F.relu followed by an in-place nn.ReLU, :245-246 --
    so gradients are compared on the plain model as in the golden test) on a 4-hop block of a Delaunay scene (the oracle materialises the
    reference's whole-scene [E_all, C] edge tensors, which bounds the scene size here): composite conv calls + sparse edge chaining against the CPU
    oracle in fp64 -- logits and every parameter gradient.
    Widths: the shipped ones, [64,128,256,512] (configs/eth.yaml:56, aerial.yaml:57) and -- round 5, BASELINE config 3 at its own workload --
    [128,256,512,1024] at batch 1024 (configs/modelnet.yaml:44,56).
    bf16 STORAGE (round 5): the gradients are held to the STORAGE-ROUNDING MODEL of tests/bf16_training_model.py -- the fp64 step
    with a round-to-bf16 at exactly the tensors the HIP path stores or feeds to the bf16 matrix cores -- within 1e-3 of each tensor's largest entry
    (two correct fp32-accumulating implementations of that model differ by 2-3.5e-4: python tests/test_bf16_rounding_model_cpu.py, `arith=`), and
    the logits to it within two bf16 steps.  The model's own distance from the un-rounded oracle is the price of the format, printed here and
    tabulated in BASELINE.md section 4 (it is set by ReLU-mask flips of near-zero pre-activations: ANY 2^-9 perturbation of the forward pass moves
    the early layers' gradients by 3-8 % rms; keeping dy / dphi in fp32 would not change it); the logits keep SURVEY 8c's tolerance against the oracle."""
    from dgnn_amd.learning import surfaceNetUpdatedEdgeFilters as U
    from dgnn_amd.sampler import NeighborSampler
    from dgnn_amd.synthetic import delaunay_tet_graph, hashed_normal
    from oracle.updated_edge_filters import SurfaceNet as ONet
    adj, _, _ = delaunay_tet_graph(points, 1)
    n = adj.shape[0] // 4
    ei = torch.from_numpy(adj.T.astype(np.int64)).to(DEV)
    x = hashed_normal(np.arange(n), 29, seed=1, device=DEV)
    ea = hashed_normal(np.arange(4 * n), 20, seed=2, device=DEV)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:batch].to(DEV)
    _, n_id, adjs = NeighborSampler(ei, sizes=[-1] * 4, num_nodes=n, batch_size=batch).sample(idx)
    assert n_id.numel() > (50000 if points >= 30000 else 20000)
    G = hashed_normal(np.arange(batch), params[-1], seed=7, device=DEV)
    clf = Config.wrap(dict(training=dict(model_params=list(params), model_name="sage", loss="kl"),
                           features=dict(normalization_feature=1, keep_normalization_feature=0), temp=dict(device=DEV)))
    oclf = Config.wrap(dict(training=dict(model_params=list(params), model_name="sage", loss="kl"),
                            features=dict(normalization_feature=1, keep_normalization_feature=0), temp=dict(device="cpu")))
    torch.manual_seed(5)
    net = U.SurfaceNet(28, clf)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net = net.to(DEV).set_storage_dtype(dtype)
    logits = net(Config(x=x, edge_attr=ea, n_id=n_id, adjs=adjs))
    (logits * G).sum().backward()
    cadjs = [(a.cpu(), e.cpu(), s) for a, e, s in adjs]
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)   # the oracle's torch.zeros([E_all, C]) (reference :236) must be fp64 too
    try:
        onet = ONet(28, oclf)
        onet.load_state_dict({k: v.double() for k, v in sd.items()})
        ologits = onet(Config(x=x.double().cpu(), edge_attr=ea.double().cpu(), n_id=n_id.cpu(), adjs=cadjs))
        (ologits * G.double().cpu()).sum().backward()
    finally:
        torch.set_default_dtype(old)
    scale = max(1.0, ologits.abs().max().item())
    err = (logits.detach().double().cpu() - ologits.detach()).abs()
    ograds = {k: p.grad for k, p in onet.named_parameters()}
    gmax = max(g.abs().max().item() for g in ograds.values())
    hgrads = {k: p.grad for k, p in net.named_parameters()}
    if dtype == torch.float32:
        assert err.max().item() <= 2e-4 * scale
        for k, g in hgrads.items():
            e = (g.double().cpu() - ograds[k]).abs().max().item()
            assert e <= 5e-4 * ograds[k].abs().max().item() + 5e-6 * gmax, (k, e, ograds[k].abs().max().item(), gmax)
        return
    # bf16 storage.  Logits against the oracle: SURVEY 8c's two-level tolerance
    assert (err <= 5e-2 * scale).float().mean().item() >= 0.9999 and err.max().item() <= 1e-1 * scale
    from bf16_training_model import error_table, updated_step
    mlogits, mgrads = updated_step(sd, params, 28, x.cpu(), ea.cpu(), n_id.cpu(), cadjs, G.cpu())
    assert set(mgrads) == set(hgrads)
    # logits against the model: the same bf16 values except where the fp32 accumulation order tips a rounding (a step of the top binade is 2^-8 of it)
    dl = (logits.detach().double().cpu() - mlogits).abs()
    top = mlogits.abs().max().item()
    assert (dl == 0).double().mean().item() >= 0.995 and dl.max().item() <= 2.0 ** -7 * top, ((dl == 0).double().mean().item(), dl.max().item(), top)
    vs_model = error_table(mgrads, hgrads)
    price = error_table(ograds, mgrads)             # the format's price: model vs the un-rounded oracle
    vs_oracle = error_table(ograds, hgrads)
    rows = []
    for l in range(len(params)):
        ks = [k for k in sorted(mgrads) if k.startswith("convs.%d." % l)]
        rows.append(dict(layer=l, hip_vs_model_max=max(vs_model[k][0] for k in ks), hip_vs_model_rms=max(vs_model[k][1] for k in ks),
                         model_vs_oracle_max=max(price[k][0] for k in ks), model_vs_oracle_rms=max(price[k][1] for k in ks),
                         hip_vs_oracle_max=max(vs_oracle[k][0] for k in ks), hip_vs_oracle_rms=max(vs_oracle[k][1] for k in ks)))
    print("bf16 training, widths %s, batch %d, block of %d cells: per conv layer (worst parameter tensor)" % (list(params), batch, n_id.numel()))
    for r in rows:
        print("   layer %(layer)d: HIP vs rounding model max %(hip_vs_model_max).2e rms %(hip_vs_model_rms).2e | price (model vs fp64 oracle) max %(model_vs_oracle_max).2e rms "
              "%(model_vs_oracle_rms).2e | HIP vs oracle max %(hip_vs_oracle_max).2e rms %(hip_vs_oracle_rms).2e" % r)
    try:      # scratch copy for BASELINE.md's table
        import json
        os.makedirs(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out"), exist_ok=True)
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "bf16_training_price_%s.json" % "_".join(map(str, params))), "w") as f:
            json.dump(dict(widths=list(params), batch=batch, block_cells=int(n_id.numel()), layers=rows), f)
    except OSError:
        pass
    # The bound.  Two CORRECT fp32-accumulating implementations of the model do not agree to fp32 rounding: where an accumulation order tips the
    # rounding of one stored bf16 value, and that value sits next to a ReLU threshold further down, one mask entry flips and with it one row's
    # contribution to the gradients below it -- sparse, row-shaped differences.  The model evaluated in fp32 against itself in fp64 (tests/
    # bf16_training_model.py `arith=`; python tests/test_bf16_rounding_model_cpu.py) shows what that amounts to: 2-5e-4 of a tensor's largest entry at
    # the shipped widths and [64,128,256,512], and at [128,256,512,1024] anything from 5e-4 to isolated entries at 2e-2 with an rms of 4e-3,
    # depending on the block -- while ONE mis-placed rounding site (a site of the model switched off) is dense: rms 3-7 % on the layers below it.
    # Hence: rms <= 1e-3 of the tensor's rms (measured here: <= 5.2e-4), all but 0.1 % of a tensor's entries (two of a bias vector) within 1e-3 of its largest (fp32 class),
    # every entry within 2e-2 (a flipped mask entry's row).
    assert_grads_within_rounding_model(mgrads, hgrads)
    # A loose guard against the un-rounded fp64 oracle stays: the rounding model is hand-written beside the kernels, so a rounding site
    # mirrored wrongly in both, or a regression that shows up as a larger format price, must not pass on the model comparison alone.  Tabulated
    # price: 8.4-9.4 % rms at layer 0, 6.5-6.8 % / 4.5-5.5 % at layers 1 / 2, 0.5-0.6 % at the last conv layer; the bound
    # is 1.5 x the worst tabulated figure per layer class, for the model AND for the HIP gradients.
    for r in rows:
        cap = 0.14 if r["layer"] < len(params) - 1 else 0.012
        assert r["model_vs_oracle_rms"] <= cap and r["hip_vs_oracle_rms"] <= cap, r
        assert abs(r["hip_vs_oracle_rms"] - r["model_vs_oracle_rms"]) <= 2e-3, r      # the HIP path pays the model's price, not more


@pytest.mark.parametrize("k1,k2,n_out", [(128, 128, 128), (64, 0, 2), (128, 0, 64), (70, 33, 37), (256, 256, 512), (28, 28, 64)])
def test_x3_gemm_small_problem_kernel_equals_the_tiled_kernels(monkeypatch, k1, k2, n_out):
    """M <= 16384 takes the no-LDS kernel (one wavefront per 32 x 32 output block, operands split in registers); same k-step and product
    order per output element as the tiled kernels, which the same rows reach when they are part of a larger problem: bit-identical."""
    from dgnn_amd import ops
    monkeypatch.setattr(ops, "GEMM_MODE", ops.GEMM_BF16X3)
    g = torch.Generator().manual_seed(k1 + 3 * n_out)
    M = 2048 + 19
    A1 = torch.randn(M, k1, generator=g).to(DEV)
    W1 = (torch.randn(n_out, k1, generator=g) / k1 ** 0.5).to(DEV)
    A2 = torch.randn(M, k2, generator=g).to(DEV) if k2 else None
    W2 = (torch.randn(n_out, k2, generator=g) / k2 ** 0.5).to(DEV) if k2 else None
    bias = torch.randn(n_out, generator=g).to(DEV)
    small = ops.linear_fwd(A1, W1, A2, W2, bias, relu=True)
    reached("x3", "X3_MID1" if n_out == 512 else "X3_SMALL", M, n_out, k1 + k2)     # (256, 256, 512): the 64 x 64 tiles took this shape over in round 6
    rep = 9                                                                  # 18603 rows: past the small-problem threshold
    big = ops.linear_fwd(A1.repeat(rep, 1), W1, A2.repeat(rep, 1) if k2 else None, W2, bias, relu=True)
    reached("x3", "X3_N64" if n_out <= 64 else "X3", rep * M, n_out, k1 + k2)
    assert torch.equal(small, big[:M]) and torch.equal(small, big[-M:])
    ref = A1.double() @ W1.double().t() + bias.double()
    if k2:
        ref = ref + A2.double() @ W2.double().t()
    assert (small.double() - ref.clamp_min(0)).abs().max().item() <= 4e-6 * max(ref.abs().max().item(), 1.0)
    acc = torch.randn(M, n_out, generator=g).to(DEV)
    out = acc.clone()
    from dgnn_amd._lib import lib, ptr, stream_ptr, check
    check(lib().dgnn_linear_fwd_x3(ptr(A1), A1.stride(0), k1, ptr(W1), k1, None, 0, 0, None, 0, None, None, None, 2, M, n_out, ptr(out), n_out, stream_ptr()), "x3")
    assert torch.equal(out, acc + ops.linear_fwd(A1, W1))


@pytest.mark.parametrize("k1,k2,n_out,M", [(512, 512, 1024, 1024), (1024, 0, 512, 2050), (1030, 77, 200, 333), (2048, 0, 64, 31)])
def test_small_gemm_split_k_form(monkeypatch, k1, k2, n_out, M):
    """Round 6: M <= 16384 rows and K = k1 + k2 >= 1024 (the reference's training widths, configs/modelnet.yaml:56: the 512 -> 1024 conv layer, the
    1024 -> 512 decoder Linear and their input gradients at batch 1024) take the small-problem kernels in their split-K form -- four wavefronts per
    32 x 32 output block, a quarter of the k-steps each, partial blocks added in wavefront order.  fp32-class arithmetic (x3) against fp64 within the
    tiled kernels' tolerance, bf16 storage against fp64 on the bf16-rounded operands at fp32-accumulation level; the same bits on a second call; ragged
    K / N / M; bias + BatchNorm + ReLU epilogue.
    What the dispatch observer shows (`form` below): the first two shapes have 128 or more 64 x 64 tiles and take those with four K groups per
    workgroup (k_linear_fwd_x3_mid<4> / k_linear_fwd_b_mid<., 4>); the last two take the split-K small-problem kernels."""
    form = "MID4" if M >= 1024 else "SMALL_SPLITK"
    from dgnn_amd import ops
    monkeypatch.setattr(ops, "GEMM_MODE", ops.GEMM_BF16X3)
    g = torch.Generator().manual_seed(k1 + 3 * n_out)
    A1 = torch.randn(M, k1, generator=g).to(DEV)
    W1 = (torch.randn(n_out, k1, generator=g) / (k1 + k2) ** 0.5).to(DEV)
    A2 = torch.randn(M, k2, generator=g).to(DEV) if k2 else None
    W2 = (torch.randn(n_out, k2, generator=g) / (k1 + k2) ** 0.5).to(DEV) if k2 else None
    bias, scale, shift = torch.randn(n_out, generator=g).to(DEV), (torch.rand(n_out, generator=g) + 0.5).to(DEV), (torch.randn(n_out, generator=g) * 0.1).to(DEV)

    def ref(a1, w1, a2, w2):
        r = a1.double() @ w1.double().t() + bias.double()
        m = a1.double().abs() @ w1.double().abs().t() + bias.double().abs()
        if a2 is not None:
            r = r + a2.double() @ w2.double().t()
            m = m + a2.double().abs() @ w2.double().abs().t()
        return (r * scale.double() + shift.double()).clamp_min(0), m * scale.double().abs() + shift.double().abs()
    got = ops.linear_fwd(A1, W1, A2, W2, bias, scale, shift, relu=True)
    reached("x3", "X3_" + form, M, n_out, k1 + k2)
    want, mag = ref(A1, W1, A2, W2)
    assert ((got.double() - want).abs() <= 2e-6 * mag + 1e-30).all(), ((got.double() - want).abs() / mag).max().item()
    assert torch.equal(got, ops.linear_fwd(A1, W1, A2, W2, bias, scale, shift, relu=True))
    # bf16 storage: operands as the kernel sees them (A bf16 as stored, W rounded to bf16 when staged), fp32 accumulate, fp32 out
    bf = lambda t: t.to(torch.bfloat16)
    A1b, A2b = bf(A1), (bf(A2) if k2 else None)
    gotb = ops.linear_fwd(A1b, W1, A2b, W2, bias, scale, shift, relu=True, out_dtype=torch.float32)
    reached("bf16", "B_" + form, M, n_out, k1 + k2)
    wantb, magb = ref(A1b.float(), bf(W1).float(), A2b.float() if k2 else None, bf(W2).float() if k2 else None)
    assert ((gotb.double() - wantb).abs() <= 4e-6 * magb + 1e-30).all(), ((gotb.double() - wantb).abs() / magb).max().item()
    assert torch.equal(gotb, ops.linear_fwd(A1b, W1, A2b, W2, bias, scale, shift, relu=True, out_dtype=torch.float32))


# Bounds of the Static bf16 step against its rounding model.  Measured spread between two CORRECT implementations of the model -- static_step in fp32
# arithmetic against itself in fp64, all sites on (tests/test_bf16_rounding_model_cpu.py::static_spread, blocks of the sizes below): worst tensor rms
# 3.3e-2 (kf96, 30 000 points / batch 2048), 3.6e-2 ([64,128,256,512]) and 4.2e-2 ([128,256,512,1024], both 10 000 / 1024); worst entry 6.7e-2 /
# 8.8e-2 / 1.5e-1 of the tensor's largest; worst single row or column rms 0.24 / 0.16 / 0.24 of the tensor's rms; logits at most 3.3e-3 / 5.2e-3 /
# 4.1e-3 of the largest; running buffers 2.7e-6 .. 6.2e-6 of their largest entry (HIP against the model: up to 7e-5 where a random-init
# running_mean is small against the z it averages).  The spread is DENSE, unlike the Updated model's: z is stored in
# bf16 AHEAD of BatchNorm, and where a channel's mean is large against its spread (kf96's decoder: |z| ~ 4e3, std ~ 6) one accumulation-order tip of
# a stored z moves the normalised value by a sizeable fraction of a std, which every gradient below sees through the batch statistics.
# What the bound sees (the model with one site family left out, against the full model, same blocks): a / w / x / y / z -- the forward families --
# move the worst tensor by 0.10-0.18 rms and a row / column by 0.34-0.96; the backward families dy / dz / da / dx / dxacc by 0.004-0.009 rms, 4-10x
# below the spread: THEY CANNOT BE SEEN by a whole-step comparison (nor on the F3 block of test_gpu_bf16.py: spread 8.6e-3, those families
# 5-10e-3); the kernel-level tests hold those stores (test_gpu_bf16.py: the generic bf16 ops and the BatchNorm sweep).  A mis-indexed channel is a whole wrong row or column: ~1x the tensor's rms along that line.  The biases ahead of a BatchNorm
# (analytically zero gradient) hold bf16 noise of up to 3.3e-4 of the model's largest gradient in that spread (the fp32 tests' floor is 5e-6): 2e-3.
from bf16_training_model import STATIC_BF16_CAP, STATIC_BF16_LINE, STATIC_BF16_RMS  # noqa: E402  (0.06, 0.3, 0.5; test_bf16_rounding_model_cpu.py holds them to the spread)


@pytest.mark.parametrize("convs,points,batch", [((64, 128, 128, 128), 30000, 2048), ((64, 128, 256, 512), 10000, 1024), ((128, 256, 512, 1024), 10000, 1024)])
def test_static_bf16_training_step_at_scale_matches_the_rounding_model(convs, points, batch):
    """The Static SurfaceNet's bf16 training step (set_storage_dtype(bf16): the per-layer dgnn_sage_layer_train_{fwd,bwd}_bf16 calls under autograd,
    the decoder's Linear + BatchNorm + ReLU through the same call without a graph, the fp32-output last Linear) on a 4-hop block built by the GPU
    NeighborSampler, against the storage-rounding model tests/bf16_training_model.py::static_step in fp64 on the CPU: logits, every parameter gradient
    (the structured bound of assert_grads_within_rounding_model with the figures above), the running buffers of every BatchNorm (tight: both take
    fp64 sums over the same bf16 z) and num_batches_tracked exactly; a loose per-layer guard against the un-rounded fp64 oracle (the price)."""
    from bf16_training_model import error_table, static_step
    from dgnn_amd.sampler import NeighborSampler
    from dgnn_amd.synthetic import delaunay_tet_graph, hashed_normal
    from test_gpu_parity import hip_static
    shipped = tuple(convs) == (64, 128, 128, 128)
    torch.set_num_threads(16)
    adj, _, _ = delaunay_tet_graph(points, 0)
    n = adj.shape[0] // 4
    ei = torch.from_numpy(adj.T.astype(np.int64)).to(DEV)
    x = hashed_normal(np.arange(n), 29, seed=1, device=DEV)
    ea = hashed_normal(np.arange(4 * n), 20, seed=2, device=DEV)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:batch].to(DEV)
    _, n_id, adjs = NeighborSampler(ei, sizes=[-1] * 4, num_nodes=n, batch_size=batch).sample(idx)
    assert n_id.numel() > (100000 if shipped else 40000)
    sd0 = None if shipped else oracle_static(convs=convs, load=False, seed=11).state_dict()
    net = hip_static(train=True, convs=convs, sd=sd0).set_storage_dtype(torch.bfloat16)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    G = hashed_normal(np.arange(batch), 2, seed=7, device=DEV)
    logits = net(Config(all=Config(x=x, edge_attr=ea), batch_n_id=n_id, batch_adjs=adjs))
    assert logits.dtype == torch.float32
    (logits * G).sum().backward()
    cadjs = [(a.cpu(), e.cpu(), s) for a, e, s in adjs]
    mlogits, mgrads, mbufs = static_step(sd, convs, x.cpu(), ea.cpu(), n_id.cpu(), cadjs, G.cpu())
    _, ograds, _ = static_step(sd, convs, x.cpu(), ea.cpu(), n_id.cpu(), cadjs, G.cpu(), sites=())     # the un-rounded step (= the oracle's autograd)
    hgrads = {k: p.grad for k, p in net.named_parameters()}
    assert set(mgrads) == set(hgrads)
    # logits: fp32 out of bf16 hidden rows -- fp32 class where no hidden value tipped, one tipped value moves a logit by a step of that value
    dl = (logits.detach().double().cpu() - mlogits).abs()
    top = mlogits.abs().max().item()
    near = (dl <= 1e-5 * top).double().mean().item()
    print("Static bf16 training, widths %s, batch %d, block of %d cells: logits vs model max %.2e of the top (%.4f within 1e-5)" % (
        list(convs), batch, n_id.numel(), dl.max().item() / top, near))
    assert dl.max().item() <= 2.0 ** -6 * top and dl.pow(2).mean().sqrt().item() <= 2.0 ** -9 * top, (dl.max().item(), top)
    # running buffers and the batch counters
    hb = dict(net.named_buffers())
    assert set(hb) == set(mbufs)
    for k, b in mbufs.items():
        if k.endswith("num_batches_tracked"):
            assert int(hb[k]) == int(b) == int(sd[k]) + 1, k
        else:
            assert (hb[k].double().cpu() - b).abs().max().item() <= 3e-4 * b.abs().max().item() + 1e-7, (k, (hb[k].double().cpu() - b).abs().max().item())
    vs_model, price, vs_oracle = error_table(mgrads, hgrads), error_table(ograds, mgrads), error_table(ograds, hgrads)
    zero = lambda k: k.endswith("conv.lin_j.bias") or k == "decoder.0.bias"        # biases ahead of a train-mode BatchNorm
    rows = []
    for l in ["convs.%d." % i for i in range(len(convs))] + ["decoder."]:
        ks = [k for k in sorted(mgrads) if k.startswith(l) and not zero(k)]
        rows.append(dict(layer=l, hip_vs_model_max=max(vs_model[k][0] for k in ks), hip_vs_model_rms=max(vs_model[k][1] for k in ks),
                         model_vs_oracle_max=max(price[k][0] for k in ks), model_vs_oracle_rms=max(price[k][1] for k in ks),
                         hip_vs_oracle_max=max(vs_oracle[k][0] for k in ks), hip_vs_oracle_rms=max(vs_oracle[k][1] for k in ks)))
    for r in rows:
        print("   %(layer)-9s HIP vs rounding model max %(hip_vs_model_max).2e rms %(hip_vs_model_rms).2e | price (model vs fp64 oracle) max %(model_vs_oracle_max).2e "
              "rms %(model_vs_oracle_rms).2e | HIP vs oracle max %(hip_vs_oracle_max).2e rms %(hip_vs_oracle_rms).2e" % r)
    assert_grads_within_rounding_model(mgrads, hgrads, rms_bound=STATIC_BF16_RMS, outside_per=None, cap=STATIC_BF16_CAP, line_bound=STATIC_BF16_LINE,
                                       zero_keys=[k for k in mgrads if zero(k)], zero_floor=2e-3)
    # the price guard: measured model-vs-oracle rms per layer 9-11 % (kf96), 13-19 % (random-init wide layers); bound 1.5x the worst, for the model
    # AND the HIP gradients, which pay the model's price plus the spread above, not more
    for r in rows:
        assert r["model_vs_oracle_rms"] <= 0.3 and r["hip_vs_oracle_rms"] <= 0.3, r
        assert abs(r["hip_vs_oracle_rms"] - r["model_vs_oracle_rms"]) <= 0.03, r
