#!/usr/bin/env python3
"""Cost of normalization 'l' (graph LayerNorm, csrc/lnorm.hip) on the MI355X.

    python tools/bench_layernorm.py model [--points 150000]   inference_layer ms/step of an 'l' model next to the shipped 'b' model
                                                              (kf96 widths and weights; the 'l' model carries the same conv / decoder
                                                              weights and LayerNorm weight 1 / bias 0) on the seeded 1M-tet scene
    python tools/bench_layernorm.py ops [--rows 1010078 --channels 128]
                                                              the LayerNorm passes alone (forward: stats, finaliser, apply; backward)
                                                              on an fp32 [rows, channels] tensor, timed with events
    python tools/bench_layernorm.py roofline <kernel_stats.csv> [--rows R --channels C]
                                                              each LayerNorm kernel's share of the 8 TB/s HBM roofline from the
                                                              `rocprofv3 --kernel-trace --stats` table of an `ops` run

Each prints one JSON line.  Bytes per kernel are what the algorithm must move (fp32 [R, C] tensors): stats reads x, apply reads x and
writes y, the backward column pass reads x and dy, the dx pass reads x and dy and writes dx.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
# kernel name fragment -> tensors of [R, C] fp32 it moves
KERNEL_TENSORS = {"k_ln_stats": 1, "k_ln_apply": 2, "k_ln_bwd_cols": 2, "k_ln_bwd_apply": 3}


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    for i in range(steps):
        evs[i].record()
        fn()
    evs[steps].record()
    torch.cuda.synchronize()
    per = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))
    return per[len(per) // 2]


def run_model(a):
    import numpy as np
    import torch
    from dgnn_amd.config import Config, reconbench_pretrained
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import SurfaceNet
    from dgnn_amd.synthetic import delaunay_tet_graph
    dev = "cuda:0"
    adj, _, _ = delaunay_tet_graph(a.points, 0)
    n = adj.shape[0] // 4
    g = torch.Generator().manual_seed(0)
    data = Config(x=torch.randn(n, 29, generator=g).to(dev), edge_attr=torch.randn(4 * n, 20, generator=g).to(dev),
                  edge_index=torch.from_numpy(adj.T.astype(np.int64)).to(dev))
    w = np.load(os.path.join(ROOT, "tests", "golden", "kf96_weights.npz"))
    sd = {k: torch.from_numpy(w[k]) for k in w.files}
    out = dict(tool="bench_layernorm", mode="model", tets=n, steps=a.steps)
    for norm in ("b", "l"):
        clf = reconbench_pretrained(device=dev)
        clf.model.normalization = norm
        net = SurfaceNet(clf)
        keys = net.state_dict().keys()
        net.load_state_dict({k: v for k, v in sd.items() if k in keys}, strict=(norm == "b"))
        net = net.to(dev).eval()
        ms = timed(lambda: net.inference_layer(data), a.steps, a.warmup)
        out["%s_ms_per_step" % norm] = round(ms, 4)
        out["%s_tets_per_s" % norm] = round(n / (ms * 1e-3), 1)
    out["l_over_b"] = round(out["l_ms_per_step"] / out["b_ms_per_step"], 3)
    print(json.dumps(out))


def run_ops(a):
    import torch
    from dgnn_amd import ops
    dev = "cuda:0"
    R, C = a.rows, a.channels
    g = torch.Generator().manual_seed(0)
    x = torch.randn(R, C, generator=g).to(dev)
    dy = torch.randn(R, C, generator=g).to(dev)
    w, b = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
    y, stats, scale = ops.graph_ln_forward(x, w, b, 1e-5, True)
    tb = R * C * 4
    fwd = timed(lambda: ops.graph_ln_forward(x, w, b, 1e-5, True), a.steps, a.warmup)
    bwd = timed(lambda: ops.graph_ln_relu_bwd(x, dy, stats, w, scale, b, True), a.steps, a.warmup)
    print(json.dumps(dict(tool="bench_layernorm", mode="ops", rows=R, channels=C, tensor_mb=round(tb / 2 ** 20, 1),
                          fwd_ms=round(fwd, 4), fwd_bytes_per_s=round(3 * tb / (fwd * 1e-3), 1),
                          bwd_ms=round(bwd, 4), bwd_bytes_per_s=round(5 * tb / (bwd * 1e-3), 1))))


def run_roofline(a):
    tb = a.rows * a.channels * 4
    rows = {}
    with open(a.csv) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            for frag, k in KERNEL_TENSORS.items():
                if frag + "<" in name or name.endswith(frag) or (frag + "(") in name or (frag + "I") in name:
                    avg_ns = float(r.get("AverageNs") or (float(r["TotalDurationNs"]) / float(r["Calls"])))
                    cur = rows.setdefault(frag, dict(calls=0, avg_us=0.0))
                    cur["calls"] += int(float(r.get("Calls", 1)))
                    cur["avg_us"] = round(avg_ns / 1e3, 2)
                    cur["bytes"] = k * tb
                    cur["hbm_share"] = round((k * tb / HBM_PEAK) / (avg_ns * 1e-9), 3)
    print(json.dumps(dict(tool="bench_layernorm", mode="roofline", rows=a.rows, channels=a.channels, hbm_peak=HBM_PEAK, kernels=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["model", "ops", "roofline"])
    ap.add_argument("csv", nargs="?")
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--rows", type=int, default=1010078)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.mode == "roofline":
        if not a.csv:
            ap.error("roofline needs the kernel_stats.csv of an `ops` run")
        return run_roofline(a)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_layernorm: no GPU (nothing is measured on the CPU)")
    (run_model if a.mode == "model" else run_ops)(a)


if __name__ == "__main__":
    main()
