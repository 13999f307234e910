"""Times the manifold repair -- ops.vertex_components (one detection pass) and ops.manifold_repair (the whole call, its host loop and
synchronisations included) -- on the scene of tools/bench_mesh_topology.py: a seeded scipy Delaunay at bench scale (150 000 points, about
1M tets), labelled by a sphere's signed distance at the centroids and by 10 % random inside labels.  ops.mesh_topology of the interface
runs next to the detection pass on the same labels, and again on the repaired labels.  One warm-up, then the median of --reps whole calls
with the range; every timing ends in a device synchronise.  Prints one JSON line per labelling.

    python tools/bench_manifold_repair.py [--points 150000] [--reps 5]
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
from dgnn_amd import ops  # noqa: E402
from dgnn_amd.processing.generate_mesh import interface_from_labels  # noqa: E402


def _time(fn, reps):
    fn()   # warm-up (code objects, allocator)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return out, dict(median=float(np.median(times)), min=min(times), max=max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_manifold_repair needs a GPU")
    scene = mm.scene_from_points(np.random.default_rng(0).random((a.points, 3)))
    dev = {k: torch.from_numpy(v).cuda() for k, v in scene.items()}
    nv, n = len(scene["vertices"]), len(scene["tetrahedra"])
    nbr, t_nbr = _time(lambda: ops.tet_neighbors(dev["facets"], dev["nfacets"], dev["tetrahedra"]), a.reps)

    def topology(labels):
        ids = interface_from_labels(labels, dev["nfacets"])
        faces, _ = ops.orient_interface(dev["vertices"], dev["tetrahedra"], dev["facets"], dev["nfacets"], labels, ids)
        return faces, ops.mesh_topology(faces, nv)

    for name, labels in (("sphere", mm.sphere_labels(scene)), ("random10", (np.random.default_rng(1).random(n) > 0.1).astype(np.int32))):
        lab = torch.from_numpy(labels).cuda()
        faces, before = topology(lab)
        _, t_topo = _time(lambda: ops.mesh_topology(faces, nv), a.reps)
        (_, _, n_singular), t_detect = _time(lambda: ops.vertex_components(dev["tetrahedra"], nbr, lab, nv), a.reps)
        (fixed, stats), t_repair = _time(lambda: ops.manifold_repair(dev["tetrahedra"], nbr, lab, nv), a.reps)
        (_, first), _ = _time(lambda: ops.manifold_repair(dev["tetrahedra"], nbr, lab, nv, max_rounds=1), 1)
        _, after = topology(fixed)
        passes = stats["rounds"] + 1            # every round detects; the last pass finds no move
        out = dict(labels=name, tets=n, vertices=nv, tet_neighbors_ms=t_nbr, mesh_topology_ms=t_topo, detection_ms=t_detect, singular=n_singular,
                   repair_ms=t_repair, repair_ms_per_pass=t_repair["median"] / passes, moves_per_round=stats["moves"] / max(stats["rounds"], 1),
                   moves_first_round=first["moves"], stuck=stats["singular_after"], **stats,
                   topology_before={k: before[k] for k in ("boundary_edges", "nonmanifold_edges", "nonmanifold_vertices", "watertight")},
                   topology_after={k: after[k] for k in ("boundary_edges", "nonmanifold_edges", "nonmanifold_vertices", "watertight")})
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
