"""Times whole-scene inference of the Updated SurfaceNet (surfaceNetUpdatedEdgeFilters.inference_layer: one library call, conv layers 1 .. 3 of the
64/128-wide model one launch each) on the 1M-tet synthetic scene (synthetic.delaunay_tet_graph(150000)) next to forward() in eval mode on the same
whole-scene adjs (the block kernels: linear -> aggregate -> chain_edges per layer), widths [64,128,128,128] and [128,256,512,1024], fp32 and bf16 storage.
Device time by events around interleaved rounds, median and minimum.  For every layer shape the one-launch form takes, the launch is also timed against
the three calls it replaces (and its edge-row traffic set against the model of DESIGN.md).  The logits of a subsample of rows are checked against the
fp64 oracle on those rows' full-neighbour 4-hop blocks.  Prints one JSON line.

    python tools/bench_updated_infer.py [--points 150000] [--rounds 7] [--check-rows 48]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import updated_inference_model as uim  # noqa: E402
from dgnn_amd import ops  # noqa: E402
from dgnn_amd.config import Config  # noqa: E402
from dgnn_amd.graph import plan_for  # noqa: E402
from dgnn_amd.synthetic import delaunay_tet_graph, hashed_normal  # noqa: E402

DEV = "cuda:0"


def timed(fns, rounds):
    """interleaved rounds of the callables -> per callable (median ms, min ms) of device time"""
    times = [[] for _ in fns]
    for f in fns:
        f()                                   # warm-up: code objects, allocator
    for _ in range(rounds):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [(float(np.median(t)), float(min(t))) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--check-rows", type=int, default=48)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_updated_infer needs a GPU")
    from dgnn_amd.learning.surfaceNetUpdatedEdgeFilters import SurfaceNet
    adj, _, _ = delaunay_tet_graph(a.points, seed=0)
    n = adj.shape[0] // 4
    ei_cpu = torch.from_numpy(adj.T.astype(np.int64))
    x_cpu, ea_cpu = hashed_normal(np.arange(n), 29, seed=1), hashed_normal(np.arange(4 * n), 2, seed=2)
    data = Config(x=x_cpu.to(DEV), edge_attr=ea_cpu.to(DEV), edge_index=ei_cpu.to(DEV))
    adjs = [(data.edge_index, torch.arange(4 * n, device=DEV), (n, n))] * 4
    whole = Config(x=data.x, edge_attr=data.edge_attr, n_id=torch.arange(n, device=DEV), adjs=adjs)
    out = dict(tets=int(n), edges=int(4 * n), rounds=a.rounds, models=[], layers=[])
    rows = np.random.default_rng(0).choice(n, size=min(a.check_rows, n), replace=False)
    for widths in ([64, 128, 128, 128], [128, 256, 512, 1024]):
        torch.manual_seed(sum(widths))
        net = SurfaceNet(28, uim.make_clf(widths, "sage+", device=DEV)).to(DEV).eval()
        sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
        oracle = uim.oracle_net(28, uim.make_clf(widths, "sage+"), sd)
        n_id, blocks = uim.khop_blocks(ei_cpu, n, rows, 4)
        ref = uim.oracle_forward(oracle, x_cpu, ea_cpu, n_id, blocks)
        for dtype in (torch.float32, torch.bfloat16):
            net.set_storage_dtype(dtype)
            with torch.no_grad():
                (one, _), (fwd, _) = timed([lambda: net.inference_layer(data), lambda: net(whole)], a.rounds)
                logits = net.inference_layer(data)
            err = (logits[torch.from_numpy(rows).to(DEV)].double().cpu() - ref).abs().max().item()
            out["models"].append(dict(widths=widths, storage="bf16" if dtype == torch.bfloat16 else "fp32", fused_layers=net.fused_layers,
                                      inference_layer_ms=one, forward_ms=fwd, tets_per_s=n / (one * 1e-3), forward_tets_per_s=n / (fwd * 1e-3),
                                      max_abs_err_vs_fp64=err, ref_abs_max=ref.abs().max().item()))
    # the launch against the three calls it replaces, per layer shape of the 64/128-wide model
    plan = plan_for(data.edge_index, n, n, hint=ops.PLAN_HINT_REFERENCE)
    parts = (plan.rowptr, plan.src, plan.eid)
    g = torch.Generator().manual_seed(1)
    for c_in, k_e, c_prev in ((64, 28, 28), (128, 64, 64), (128, 128, 128)):
        if not ops.edge_chain_aggregate_supported(c_in, k_e):
            continue
        x = torch.randn(n, c_in, generator=g).to(DEV)
        ea = torch.randn(4 * n, c_prev, generator=g).to(DEV)
        We, be = (torch.randn(c_in, k_e, generator=g) * 0.1).to(DEV), torch.randn(c_in, generator=g).to(DEV)
        nxt = torch.empty(4 * n, c_in, device=DEV)

        def fused(write=True):
            ops.edge_chain_aggregate_fwd(*parts, n, x, ea, We, be, ea_next=nxt, write_next=write)

        def unfused():
            phi = ops.linear_fwd(ea[:, :k_e], We, bias=be)
            ops.aggregate_fwd(*parts, n, x, phi=phi)
            ops.relu(phi)
        (f_ms, f_min), (l_ms, _), (u_ms, u_min) = timed([fused, lambda: fused(False), unfused], a.rounds)
        moved = 4 * n * 4 * (k_e + c_in)          # edge rows read + written by the launch
        out["layers"].append(dict(c_in=c_in, k_e=k_e, fused_ms=f_ms, fused_min_ms=f_min, fused_last_layer_ms=l_ms, unfused_ms=u_ms, unfused_min_ms=u_min,
                                  edge_row_gb=moved / 1e9, fused_edge_row_tb_s=moved / (f_ms * 1e-3) / 1e12))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
