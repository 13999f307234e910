"""Times the exact device graph cut (ops.binary_graph_cut) on the 1M-cell synthetic scene (synthetic.delaunay_tet_graph(150000),
finite-finite facets only) with two logit fields -- i.i.d. N(0, 2^2) noise (the hard case) and a sphere's signed distance at the cell
centroids plus the same noise (closer to real predictions) -- next to scipy's Dinic maximum flow (+ the residual BFS) on the host CPU.
Prints one JSON line per field; the labels of the two solvers are compared.

With --binary-term area / beta the facets are weighed by their geometry (ops.facet_cut_terms on the same Delaunay scene in `_3dt.npz`
layout, tests/mesh_metrics_model.random_scene: the same points, cells and facet graph, the rows in facet order) and the cut is
ops.weighted_graph_cut.  First one JSON line for the terms kernel (time, compulsory and scratch bytes, bytes/s of each), then per field the weighted
cut next to the cut with the constant weight rint(bw) on the SAME rows (`uniform_*`: what the weights themselves cost).

    python tools/bench_graph_cut.py [--points 150000] [--reps 5] [--uw 10] [--bw 1] [--no-cpu] [--binary-term {uniform,area,beta}]
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


def _timed(fn, reps):
    out = fn()                                  # warm-up (code objects, allocator)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()                              # every op here ends in a synchronising read
        times.append(time.perf_counter() - t0)
    return out, times


def terms_bytes(scene, kind, with_q):
    """-> (compulsory, scratch) bytes of dgnn_facet_cut_terms.  Compulsory: every facet's nfacets and facets rows and its outputs; per graph
    row the three vertices (area) or, for beta, two cells' vertex ids and their eight vertices (the facet's three are among them).
    Scratch (area only): A_f written, read by the sum and read by the quantise pass, and the nfacets row read again there."""
    f = len(scene["facets"])
    rows = int((scene["nfacets"] >= 0).all(axis=1).sum())
    out = f * (4 + (8 if with_q else 0))
    if kind == "area":
        return f * (8 + 12) + rows * 3 * 24 + out, f * (8 + 8 + 8 + 8)
    return f * (8 + 12) + rows * (2 * 16 + 8 * 24) + out, 0


def main_weighted(a):
    import graph_cut_weights_model as gwm
    import mesh_metrics_model as mmm

    scene = mmm.random_scene(a.points, seed=0)
    rows = gwm.graph_rows(scene["nfacets"])
    edges = np.ascontiguousarray(scene["nfacets"][rows], dtype=np.int32)
    cent, nf = mmm.centroids(scene), len(scene["tetrahedra"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(scene[k])).cuda() for k in ("vertices", "tetrahedra", "facets", "nfacets")}
    e_dev, rows_dev = torch.from_numpy(edges).cuda(), torch.from_numpy(rows).cuda()
    for with_q in (False, True):
        (w_all, *_, st), times = _timed(lambda: ops.facet_cut_terms(dev["vertices"], dev["tetrahedra"], dev["facets"], dev["nfacets"], a.binary_term,
                                                                    a.bw, return_q=with_q), a.reps)
        nbytes, scratch_bytes = terms_bytes(scene, a.binary_term, with_q)
        print(json.dumps(dict(op="facet_cut_terms", kind=a.binary_term, with_q=with_q, facets=len(rows), bw=a.bw, call_ms_median=1e3 * float(np.median(times)),
                              call_ms_min=1e3 * min(times), compulsory_bytes=nbytes, scratch_bytes=scratch_bytes, compulsory_gbytes_per_s_of_min=nbytes / min(times) / 1e9,
                              moved_gbytes_per_s_of_min=(nbytes + scratch_bytes) / min(times) / 1e9, **st)), flush=True)
    weights = w_all[rows_dev].contiguous()
    const = torch.full_like(weights, int(np.rint(a.bw)))
    for field in ("noise", "coherent"):
        pred = gcm.noise_logits(nf, seed=0) if field == "noise" else gcm.coherent_logits(cent, seed=0)
        p_dev = torch.from_numpy(pred).cuda()
        (lab, energy, flow, stats), times = _timed(lambda: ops.weighted_graph_cut(p_dev, e_dev, a.uw, weights, return_stats=True), a.reps)
        (_, _, _, ustats), utimes = _timed(lambda: ops.weighted_graph_cut(p_dev, e_dev, a.uw, const, return_stats=True), a.reps)
        out = dict(field=field, binary_term=a.binary_term, cells=int(nf), facets=int(len(edges)), uw=a.uw, bw=a.bw, gpu_ms_median=1e3 * float(np.median(times)),
                   gpu_ms_min=1e3 * min(times), steps=stats["steps"], relabels=stats["relabels"], energy=energy, flow=flow,
                   uniform_gpu_ms_median=1e3 * float(np.median(utimes)), uniform_gpu_ms_min=1e3 * min(utimes), uniform_steps=ustats["steps"],
                   uniform_relabels=ustats["relabels"])
        if not a.no_cpu:
            t0 = time.perf_counter()
            want, e_want, f_want = gwm.solve_weighted(pred, edges, a.uw, weights.cpu().numpy())
            out["cpu_dinic_s"] = time.perf_counter() - t0
            out["labels_equal"] = bool(np.array_equal(lab.cpu().numpy(), want)) and e_want == energy and f_want == flow
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--uw", type=float, default=10.0)
    ap.add_argument("--bw", type=float, default=1.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--binary-term", choices=("uniform", "area", "beta"), default="uniform")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_graph_cut needs a GPU")
    if a.binary_term != "uniform":
        return main_weighted(a)
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
