"""The whole-graph branch of the edge total-variation regulariser (what Trainer.inference with has_label pays per validated scene; reference
learning/runModel.py:109-160 on data.edge_index, E = 4N) replayed on the synthetic scene of bench.py: the library path (ops.edge_tv_fwd without a
gradient, ops.edge_tv_step with one) against the reference's torch op chain, which is what the trainer ran before csrc/edge_tv.hip, and the index
stream's rate against a device-to-device copy on the same GPU.

    python tools/bench_edge_tv.py [--points P] [--rounds R] [--iters K]

One JSON line per round and edge_index layout; the two paths alternate inside every round (interleaved: both see the same clocks)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from dgnn_amd import ops
from dgnn_amd.synthetic import delaunay_tet_graph

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=150000, help="150000 points -> ~1M tetrahedra, E = 4N")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--weight", type=float, default=0.4)
args = ap.parse_args()

dev = "cuda:0"
adj, _, _ = delaunay_tet_graph(args.points, 0)
n = adj.shape[0] // 4
pairs = torch.from_numpy(adj.astype(np.int64)).to(dev)          # [E, 2]
layouts = {"transposed view of [E, 2] (the scene loader's)": pairs.t(), "contiguous [2, E]": pairs.t().contiguous()}
E = pairs.size(0)
logits = torch.randn(n, 2, device=dev, generator=torch.Generator(dev).manual_seed(0)) * 2
w = args.weight


def timed(f, it=args.iters, warm=5):
    for _ in range(warm):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(it):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it


def chain(ei):      # reference learning/runModel.py:121-160, value and metric sum
    inner = F.softmax(logits, dim=-1)
    tv = torch.abs(inner[ei[0, :]][:, 0] - inner[ei[1, :]][:, 0])
    reg = tv * w
    return reg.sum(), reg.mean()


buf = torch.empty(E * 2, dtype=torch.int64, device=dev)
dst = torch.empty_like(buf)
for rnd in range(args.rounds):
    t_copy = timed(lambda: dst.copy_(buf))
    copy_gbs = 2 * buf.numel() * 8 / t_copy / 1e6          # bytes read + bytes written
    for name, ei in layouts.items():
        t_torch = timed(lambda: chain(ei))
        t_dev = timed(lambda: ops.edge_tv_fwd(logits, ei, w, need_grad=False))
        t_step = timed(lambda: ops.edge_tv_step(logits, ei, w))
        reg, sums, _ = ops.edge_tv_fwd(logits, ei, w, need_grad=False)
        ref = chain(ei)[1]
        print(json.dumps({"round": rnd, "edge_index": name, "tets": n, "edges": E, "library_fwd_ms": round(t_dev, 4), "library_fwd_bwd_ms": round(t_step, 4),
                          "torch_chain_fwd_ms": round(t_torch, 4), "speedup_fwd": round(t_torch / t_dev, 2), "index_bytes": E * 16,
                          "index_stream_GBps": round(E * 16 / t_dev / 1e6, 1), "copy_GBps_read_plus_write": round(copy_gbs, 1),
                          "share_of_copy_bandwidth": round(E * 16 / t_dev / 1e6 / copy_gbs, 3),
                          "rel_diff_vs_chain": abs(reg.item() - ref.item()) / ref.item()}), flush=True)
