"""Times ops.cell_labels (the fused call: no sample point goes to memory) next to the composed path (ops.tet_sample_points, then
ops.mesh_contains, then a torch reduction over [T, k]) in one process, on the Delaunay tetrahedralization of uniform points in the unit
cube (about 1e6 tets at the default 150 000 points) against a closed latitude / longitude sphere of about 1e5 triangles (radius 0.4 about
the cube's centre) at k = 100 samples per tet; and next to the host time of the numpy model (tests/cell_labels_model.py) on the first
tets that straddle the sphere, whose counts the device result is checked against.  The two device paths alternate inside the timed loop; every timing ends in a
device synchronise and covers the whole Python call (validation, plan, grid build, the kernel, the status reads).  Prints one JSON line.

    python tools/bench_cell_labels.py [--points 150000] [--samples 100] [--rings 158] [--reps 5] [--model-tets 30]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cell_labels_model as cl  # noqa: E402
from bench_mesh_contains import uv_sphere  # noqa: E402
from dgnn_amd import ops  # noqa: E402


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def _stats(ms):
    return [round(float(np.median(ms)), 3), round(min(ms), 3), round(max(ms), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--rings", type=int, default=158)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model-tets", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cell_labels needs a GPU")
    from scipy.spatial import Delaunay

    k = a.samples
    pts = np.random.default_rng(a.seed).random((a.points, 3))
    t0 = time.perf_counter()
    tets = Delaunay(pts).simplices.astype(np.int32)
    delaunay_s = time.perf_counter() - t0
    mv, mf = uv_sphere(a.rings)
    mv = mv + 0.5
    v, td, mvd, mfd = (torch.from_numpy(x).cuda() for x in (pts, tets, mv, mf))
    n_tets = len(tets)

    def fused():
        return ops.cell_labels(mvd, mfd, v, td, n_samples=k, seed=a.seed)

    composed_ms = {"sample": [], "contains": [], "reduce": []}

    def composed(record=True):
        p, t_s = _clock(lambda: ops.tet_sample_points(v, td, k, seed=a.seed))
        (occ, dis), t_c = _clock(lambda: ops.mesh_contains(mvd, mfd, p))
        cnt, t_r = _clock(lambda: occ.view(n_tets, k).sum(dim=1).to(torch.int32))
        if record:
            for key, t in (("sample", t_s), ("contains", t_c), ("reduce", t_r)):
                composed_ms[key].append(t)
        return cnt, dis

    lab = fused()                      # warm-up of both paths (code objects, allocator)
    cnt, dis = composed(record=False)
    fused_ms = []
    for _ in range(a.reps):            # alternating: whatever else the host does falls on both
        fused_ms.append(_clock(fused)[1])
        composed()
    total = [s + c + r for s, c, r in zip(composed_ms["sample"], composed_ms["contains"], composed_ms["reduce"])]
    count = lab["count"]
    res = {"tets": n_tets, "samples_per_tet": k, "mesh_triangles": len(mf), "delaunay_host_s": round(delaunay_s, 2),
           "fused_ms_median_min_max": _stats(fused_ms), "composed_ms_median_min_max": _stats(total),
           "composed_sample_ms": _stats(composed_ms["sample"]), "composed_contains_ms": _stats(composed_ms["contains"]),
           "composed_reduce_ms": _stats(composed_ms["reduce"]), "composed_points_bytes": 24 * n_tets * k,
           "fused_equals_composed": bool(torch.equal(cnt, count) and dis == lab["n_disagree"]), "n_disagree": lab["n_disagree"],
           "cells_outside": int((count == 0).sum()), "cells_inside": int((count == k).sum()),
           "mean_inside_perc": round(float(lab["inside_perc"].mean()), 4)}
    # the model on the first tets that straddle the sphere (centroid within 0.01 of it): the ones whose count is neither 0 nor k
    near = np.nonzero(np.abs(np.linalg.norm(pts[tets].mean(axis=1) - 0.5, axis=1) - 0.4) < 0.01)[0][:max(a.model_tets, 0)]
    if len(near):
        t0 = time.perf_counter()
        want = np.array([cl.labels(mv, mf, pts, tets[t:t + 1], k, a.seed, tet_offset=int(t))[0][0] for t in near])
        got = count[torch.from_numpy(near).cuda()].cpu().numpy()
        res.update(model_tets=len(near), model_host_ms=round(1e3 * (time.perf_counter() - t0), 1), model_equal=bool(np.array_equal(want, got)),
                   model_tets_partial=int(((want > 0) & (want < k)).sum()))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
