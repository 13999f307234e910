"""Times the device mesh of `generate` with ``mesh.solver: gpu`` -- ops.orient_interface + ops.compact_vertices + ops.mesh_topology --
on a seeded scipy Delaunay scene at bench scale (150 000 points, about 1M tets), labelled by a sphere's signed distance at the centroids
and by 10 % random inside labels, next to the CPU oracle (tests/mesh_topology_model.py: numpy orientation with Fractions where fp64 is
not sure, np.unique compaction, dictionary counts).  The device results are checked against the oracle.  Prints one JSON line per
labelling; every timing ends in a device synchronise.

    python tools/bench_mesh_topology.py [--points 150000] [--reps 5] [--no-cpu]
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

import mesh_metrics_model as mm  # noqa: E402
import mesh_topology_model as mt  # noqa: E402
from dgnn_amd import ops  # noqa: E402


def _time(fn, reps):
    fn()   # warm-up (code objects, allocator)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, 1e3 * float(np.median(times)), 1e3 * min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_topology needs a GPU")
    scene = mm.scene_from_points(np.random.default_rng(0).random((a.points, 3)))
    dev = {k: torch.from_numpy(v).cuda() for k, v in scene.items()}
    nv, n = len(scene["vertices"]), len(scene["tetrahedra"])
    for name, labels in (("sphere", mm.sphere_labels(scene)), ("random10", (np.random.default_rng(1).random(n) > 0.1).astype(np.int32))):
        ids = mm.interface_ids(labels, scene["nfacets"])
        lab_dev, ids_dev = torch.from_numpy(labels).cuda(), torch.from_numpy(ids).cuda()
        stage = {}

        def orient():
            return ops.orient_interface(dev["vertices"], dev["tetrahedra"], dev["facets"], dev["nfacets"], lab_dev, ids_dev)
        (faces, und), stage["orient"], _ = _time(orient, a.reps)
        (fc, kept), stage["compact"], _ = _time(lambda: ops.compact_vertices(faces, nv), a.reps)
        top, stage["topology"], _ = _time(lambda: ops.mesh_topology(fc, kept.numel()), a.reps)

        def all_three():
            f, _ = orient()
            c, k = ops.compact_vertices(f, nv)
            return ops.mesh_topology(c, k.numel())
        _, total_med, total_min = _time(all_three, a.reps)
        out = dict(labels=name, tets=n, interface_faces=len(ids), kept_vertices=int(kept.numel()), n_undetermined=und, **top,
                   gpu_orient_ms_median=stage["orient"], gpu_compact_ms_median=stage["compact"], gpu_topology_ms_median=stage["topology"],
                   gpu_total_ms_median=total_med, gpu_total_ms_min=total_min)
        if not a.no_cpu:
            t0 = time.perf_counter()
            want, want_und = mt.orient_interface(scene, labels, ids)
            want_fc, want_kept = mt.compact(want)
            want_top = mt.topology(want_fc)
            out["cpu_oracle_ms"] = 1e3 * (time.perf_counter() - t0)
            out["matches_oracle"] = bool(np.array_equal(faces.cpu().numpy(), want) and und == want_und and
                                         np.array_equal(fc.cpu().numpy(), want_fc) and np.array_equal(kept.cpu().numpy(), want_kept) and top == want_top)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
