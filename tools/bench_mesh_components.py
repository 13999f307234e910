"""Times the device mesh components -- ops.mesh_components, ops.mesh_component_measures, ops.filter_components -- on the interface of a
seeded scipy Delaunay scene at bench scale (150 000 points, about 1M tets), labelled by a sphere's signed distance at the centroids (one
large shell) and by 10 % random inside labels (thousands of small pieces), and on a shuffled strip of 1M faces (one component), next to scipy.sparse.csgraph.connected_components on the same
face-adjacency matrix on the host (tests/mesh_components_model.py; timed without and with building the matrix).  The device labels and
counts are checked against the host's.  Prints one JSON line per labelling; every device timing ends in a device synchronise.

    python tools/bench_mesh_components.py [--points 150000] [--reps 5]
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

import mesh_components_model as mc  # noqa: E402
import mesh_metrics_model as mm  # noqa: E402
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


def _host_time(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, 1e3 * float(np.median(times))


def main():
    from scipy.sparse.csgraph import connected_components

    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_components needs a GPU")
    scene = mm.scene_from_points(np.random.default_rng(0).random((a.points, 3)))
    n = len(scene["tetrahedra"])
    cases = [(name, scene["vertices"], np.ascontiguousarray(scene["facets"][mm.interface_ids(labels, scene["nfacets"])]))
             for name, labels in (("sphere", mm.sphere_labels(scene)), ("random10", (np.random.default_rng(1).random(n) > 0.1).astype(np.int32)))]
    cases.append(("strip1m",) + mc.strip(1_000_000, seed=2))       # not an interface: ONE component of 1M faces, the serial sums' worst case
    for name, vertices, faces in cases:
        nv = len(vertices)
        v_dev, f_dev = torch.from_numpy(vertices).cuda(), torch.from_numpy(faces).cuda()
        (comp, k), t_comp, _ = _time(lambda: ops.mesh_components(f_dev, nv), a.reps)
        meas, t_meas, _ = _time(lambda: ops.mesh_component_measures(v_dev, f_dev, comp, k), a.reps)
        (kept, keep, n_kept), t_keep, _ = _time(lambda: ops.filter_components(f_dev, comp, meas["n_faces"], largest=True), a.reps)

        def all_three():
            c, kk = ops.mesh_components(f_dev, nv)
            m = ops.mesh_component_measures(v_dev, f_dev, c, kk)
            return ops.filter_components(f_dev, c, m["n_faces"], largest=True)
        _, total_med, total_min = _time(all_three, a.reps)
        adj, t_adj = _host_time(lambda: mc.face_adjacency(faces), a.reps)
        (_, lab), t_cc = _host_time(lambda: connected_components(adj, directed=False), a.reps)
        want, want_k = mc.renumber(lab)
        counts = np.bincount(want, minlength=want_k)
        out = dict(labels=name, tets=n, faces=len(faces), components=k, largest_component_faces=int(n_kept),
                   gpu_components_ms_median=t_comp, gpu_measures_ms_median=t_meas, gpu_filter_ms_median=t_keep, gpu_total_ms_median=total_med,
                   gpu_total_ms_min=total_min, host_adjacency_ms_median=t_adj, host_connected_components_ms_median=t_cc,
                   matches_host=bool(k == want_k and np.array_equal(comp.cpu().numpy(), want) and
                                     np.array_equal(meas["n_faces"].cpu().numpy(), counts) and n_kept == int(counts.max())))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
