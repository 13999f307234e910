"""Times ops.mesh_contains for 100 000 query points (the reference's points_size) against closed meshes of about 1e4, 1e5 and 1e6
triangles (latitude / longitude spheres of radius 0.4 about the origin, points uniform in the unit box), next to the host time of the
all-pairs numpy model (tests/mesh_contains_model.py) at a size it can finish, whose answer the device result is checked against.
Prints one JSON line per mesh; every device timing ends in a device synchronise and covers the whole call (validation, grid build,
query, the two status reads).

    python tools/bench_mesh_contains.py [--points 100000] [--reps 5] [--model-points 2000]
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

import mesh_contains_model as mc  # noqa: E402
from dgnn_amd import ops  # noqa: E402


def uv_sphere(rings, radius=0.4):
    """closed sphere of 2 * segments * (rings - 1) triangles, segments = 2 * rings"""
    seg = 2 * rings
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(seg) / seg
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(seg))], -1).reshape(-1, 3)
    v = radius * np.concatenate([ring, [[0, 0, 1], [0, 0, -1]]])
    top, bot = len(ring), len(ring) + 1
    i, j = np.meshgrid(np.arange(rings - 2), np.arange(seg), indexing="ij")
    a, b, c, d = i * seg + j, i * seg + (j + 1) % seg, (i + 1) * seg + j, (i + 1) * seg + (j + 1) % seg
    quads = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    j = np.arange(seg)
    caps = np.concatenate([np.stack([np.full(seg, top), j, (j + 1) % seg], -1),
                           np.stack([np.full(seg, bot), (rings - 2) * seg + (j + 1) % seg, (rings - 2) * seg + j], -1)])
    return v, np.concatenate([quads, caps]).astype(np.int32)


def _time(fn, reps):
    fn()   # warm-up (code objects, allocator)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, 1e3 * float(np.median(times)), 1e3 * min(times), 1e3 * max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model-points", type=int, default=2000)
    ap.add_argument("--rings", type=int, nargs="+", default=[50, 158, 500])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_contains needs a GPU")
    pts = ops.box_points(a.points, 1.0, seed=0)
    for rings in a.rings:
        v, f = uv_sphere(rings)
        vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
        (occ, n_disagree), med, lo, hi = _time(lambda: ops.mesh_contains(vd, fd, pts), a.reps)
        topo = ops.mesh_topology(fd, len(v))
        res = {"triangles": len(f), "points": a.points, "device_ms_median": round(med, 3), "device_ms_min": round(lo, 3), "device_ms_max": round(hi, 3),
               "inside": int(occ.sum()), "n_disagree": n_disagree, "closed": bool(topo["boundary_edges"] == 0 and topo["nonmanifold_edges"] == 0),
               "sphere_volume_share": round(4 / 3 * np.pi * 0.4 ** 3, 4)}
        m = min(a.model_points, a.points)
        if m > 0 and len(f) * m <= 3e8:                      # pairs the numpy model finishes in well under a minute
            sub = pts[:m].cpu().numpy()
            t0 = time.perf_counter()
            want, want_dis = mc.contains(v, f, sub)
            res.update(model_points=m, model_host_ms=round(1e3 * (time.perf_counter() - t0), 1),
                       model_equal=bool(np.array_equal(want, occ[:m].cpu().numpy())))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
