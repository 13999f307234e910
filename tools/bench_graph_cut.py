"""Times the exact device graph cut (ops.binary_graph_cut) on the 1M-cell synthetic scene (synthetic.delaunay_tet_graph(150000),
finite-finite facets only) with two logit fields -- i.i.d. N(0, 2^2) noise (the hard case) and a sphere's signed distance at the cell
centroids plus the same noise (closer to real predictions) -- next to scipy's Dinic maximum flow (+ the residual BFS) on the host CPU.
Prints one JSON line per field; the labels of the two solvers are compared.

    python tools/bench_graph_cut.py [--points 150000] [--reps 5] [--uw 10] [--bw 1] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import graph_cut_model as gcm  # noqa: E402
from dgnn_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--uw", type=float, default=10.0)
    ap.add_argument("--bw", type=float, default=1.0)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_graph_cut needs a GPU")
    edges, cent, nf = gcm.delaunay_facet_graph(a.points, seed=0)
    e_dev = torch.from_numpy(edges).cuda()
    for field in ("noise", "coherent"):
        pred = gcm.noise_logits(nf, seed=0) if field == "noise" else gcm.coherent_logits(cent, seed=0)
        p_dev = torch.from_numpy(pred).cuda()
        lab, energy, flow, stats = ops.binary_graph_cut(p_dev, e_dev, a.uw, a.bw, return_stats=True)   # warm-up (code objects, allocator)
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lab, energy, flow, stats = ops.binary_graph_cut(p_dev, e_dev, a.uw, a.bw, return_stats=True)   # ends in a synchronising read
            times.append(time.perf_counter() - t0)
        out = dict(field=field, cells=int(nf), facets=int(len(edges)), uw=a.uw, bw=a.bw, gpu_ms_median=1e3 * float(np.median(times)),
                   gpu_ms_min=1e3 * min(times), steps=stats["steps"], relabels=stats["relabels"], energy=energy, flow=flow)
        if not a.no_cpu:
            t0 = time.perf_counter()
            want, e_want, f_want = gcm.solve(pred, edges, a.uw, a.bw)
            out["cpu_dinic_s"] = time.perf_counter() - t0
            out["labels_equal"] = bool(np.array_equal(lab.cpu().numpy(), want)) and e_want == energy and f_want == flow
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
