"""Times the device mesh metrics (ops.mesh_iou, ops.sample_interface + ops.chamfer_distance) on a seeded scipy Delaunay scene at bench
scale (150 000 points, about 1M tets) labelled by a sphere's signed distance at the centroids, next to the CPU baseline: scipy's
Delaunay.find_simplex + labels for IoU, cKDTree both ways for chamfer.  Sizes: ONet's files (100 000 occupancy points, 100 000 GT
surface points) and a larger case.  Two harder shapes follow at ONet's sizes: "far" times the nearest-neighbour search for query points
spread over the whole padded box against a sphere-surface set (recon samples far from the GT surface, as early in training), and "slab"
times IoU on a scene whose points fill a thin diagonal slab (most of the vertex box holds no cell, so most start bins are empty).  Prints
one JSON line per case; every timing ends in a device synchronise.

    python tools/bench_mesh_metrics.py [--points 150000] [--sizes 100000,2000000] [--reps 5] [--no-cpu]
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
    ap.add_argument("--sizes", default="100000,2000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_metrics needs a GPU")
    rng = np.random.default_rng(0)
    pts = rng.random((a.points, 3))
    scene = mm.scene_from_points(pts)
    labels = mm.sphere_labels(scene)
    ids = mm.interface_ids(labels, scene["nfacets"])
    dev = {k: torch.from_numpy(v).cuda() for k, v in scene.items()}
    lab_dev, ids_dev = torch.from_numpy(labels).cuda(), torch.from_numpy(ids).cuda()
    for size in (int(s) for s in a.sizes.split(",")):
        q = (rng.random((size, 3)) * 1.1 - 0.05).astype(np.float32)
        gt_occ = np.linalg.norm(q - 0.5, axis=1) < 0.3
        p = rng.normal(size=(size, 3))
        gt_pts = (0.5 + 0.3 * p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)
        q_dev, occ_dev, gt_dev = torch.from_numpy(q).cuda(), torch.from_numpy(gt_occ).cuda(), torch.from_numpy(gt_pts).cuda()
        (iou, _, _, _), iou_med, iou_min = _time(lambda: ops.mesh_iou(dev["vertices"], dev["tetrahedra"], dev["facets"], dev["nfacets"], lab_dev,
                                                                      q_dev, occ_dev), a.reps)
        _, steps = ops.locate_points(dev["vertices"], dev["tetrahedra"], dev["facets"], dev["nfacets"], q_dev, return_steps=True)

        def chamfer():
            rc, _ = ops.sample_interface(dev["vertices"], dev["facets"], ids_dev, size, seed=0)
            return ops.chamfer_distance(gt_dev, rc), rc
        (ch, rc), ch_med, ch_min = _time(chamfer, a.reps)
        out = dict(tets=len(scene["tetrahedra"]), interface_faces=len(ids), points=size, iou=iou, max_walk_steps=steps, chamfer=ch,
                   gpu_iou_ms_median=iou_med, gpu_iou_ms_min=iou_min, gpu_chamfer_ms_median=ch_med, gpu_chamfer_ms_min=ch_min)
        if not a.no_cpu:
            from scipy.spatial import Delaunay
            tri = Delaunay(pts)
            t0 = time.perf_counter()
            s = tri.find_simplex(q.astype(np.float64))
            want_iou = mm.iou((s >= 0) & (labels[np.maximum(s, 0)] == 0), gt_occ)
            out["cpu_iou_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            want_ch = mm.chamfer_ckdtree(gt_pts, rc.cpu().numpy())
            out["cpu_chamfer_s"] = time.perf_counter() - t0
            out["iou_cpu"], out["chamfer_rel_diff"] = want_iou, abs(ch - want_ch) / want_ch
        print(json.dumps(out), flush=True)

    n = 100000
    p = rng.normal(size=(n, 3))
    gt_pts = torch.from_numpy((0.5 + 0.3 * p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)).cuda()
    far = torch.from_numpy((rng.random((n, 3)) * 1.1 - 0.05).astype(np.float32)).cuda()
    (_, _, s_far), nn_med, nn_min = _time(lambda: ops.nearest_neighbor(gt_pts, far), a.reps)
    out = dict(case="far", points=n, gpu_nn_ms_median=nn_med, gpu_nn_ms_min=nn_min, mean_dist=s_far / n)
    if not a.no_cpu:
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        d, _ = cKDTree(gt_pts.cpu().numpy()).query(far.cpu().numpy())
        out["cpu_ckdtree_s"], out["mean_dist_rel_diff"] = time.perf_counter() - t0, abs(s_far / n - d.mean()) / d.mean()
    print(json.dumps(out), flush=True)

    uv = rng.random((a.points, 2))
    slab_pts = np.stack([uv[:, 0], uv[:, 1], 0.5 * (uv[:, 0] + uv[:, 1]) + 0.02 * rng.random(a.points)], axis=1)
    slab = mm.scene_from_points(slab_pts)
    slab_labels = (np.linalg.norm(mm.centroids(slab)[:, :2] - 0.5, axis=1) > 0.3).astype(np.int32)
    sdev = {k: torch.from_numpy(v).cuda() for k, v in slab.items()}
    q = (rng.random((n, 3)) * 1.1 - 0.05).astype(np.float32)
    gt_occ = np.linalg.norm(q[:, :2] - 0.5, axis=1) < 0.3
    q_dev, occ_dev, lab_dev = torch.from_numpy(q).cuda(), torch.from_numpy(gt_occ).cuda(), torch.from_numpy(slab_labels).cuda()
    (iou, _, _, _), iou_med, iou_min = _time(lambda: ops.mesh_iou(sdev["vertices"], sdev["tetrahedra"], sdev["facets"], sdev["nfacets"], lab_dev,
                                                                  q_dev, occ_dev), a.reps)
    _, steps = ops.locate_points(sdev["vertices"], sdev["tetrahedra"], sdev["facets"], sdev["nfacets"], q_dev, return_steps=True)
    out = dict(case="slab", tets=len(slab["tetrahedra"]), points=n, iou=iou, max_walk_steps=steps, gpu_iou_ms_median=iou_med, gpu_iou_ms_min=iou_min)
    if not a.no_cpu:
        from scipy.spatial import Delaunay
        s = Delaunay(slab_pts).find_simplex(q.astype(np.float64))
        out["iou_cpu"] = mm.iou((s >= 0) & (slab_labels[np.maximum(s, 0)] == 0), gt_occ)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
