"""From a raw scan to a scene folder: what a user with points and sensor positions, and no ground-truth mesh, starts from -- the
arrays of the reference's `scan/<name>.npz` (processing/reconbench/ply2npz.py, processing/eth3d/feat.py).

clean_scan removes the statistical outliers (ops.outlier_mask) and estimates the normals the reference's scan files carry (ops.estimate_normals,
turned towards each point's sensor); scene_from_scan chains it with triangulate_scan and build_scene_features and writes the `_labels.npz` the
loader opens.  A scan has no labels: that file holds `infinite` alone, which is all dataLoader.run reads of it with inference.has_label off; a
training run on such a folder fails on the missing key.  make_scene (a scene from a ground-truth mesh) is in triangulate.py.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import ops


def clean_scan(points, sensor_position, outlier_k=16, std_ratio=2.0, normals_k=16, device=None):
    """points, sensor_position [P, 3] -> dict: "points", "sensor_position", "normals" fp64 of the kept points, in input order; "kept" int64: their
    input rows; "stats": those of ops.outlier_mask with mean_distance on the host (None when std_ratio is None: nothing is removed)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    s = np.ascontiguousarray(sensor_position, dtype=np.float64).reshape(-1, 3)
    if len(p) != len(s):
        raise ValueError("clean_scan: %d sensor positions for %d points" % (len(s), len(p)))
    dp, ds = torch.from_numpy(p).to(dev), torch.from_numpy(s).to(dev)
    stats = None
    kept = np.arange(len(p), dtype=np.int64)
    if std_ratio is not None:
        keep, stats = ops.outlier_mask(dp, k=outlier_k, std_ratio=std_ratio)
        stats = dict(stats, mean_distance=stats["mean_distance"].cpu().numpy())
        kept = np.nonzero(keep.cpu().numpy())[0].astype(np.int64)
        sel = torch.from_numpy(kept).to(dev)
        dp, ds = dp[sel].contiguous(), ds[sel].contiguous()
    normals, _ = ops.estimate_normals(dp, k=normals_k, sensors=ds)
    return dict(points=p[kept], sensor_position=s[kept], normals=normals.cpu().numpy(), kept=kept, stats=stats)


def scene_from_scan(points, sensor_position, out_base, clean=True, facet_rays=False, facet_geometry=False, scan_file=None, device=None, **clean_args):
    """A raw scan -> every file dataLoader.run opens with inference.has_label off: clean_scan(**clean_args) (clean=False: the scan as it is, no
    normals) -> triangulate_scan -> build_scene_features, written as out_base + "_3dt.npz", "_adjacencies.npz", "_cgeom.npz", "_cbvf.npz",
    "_fbvf.npz" and "_labels.npz" (the key `infinite` only); facet_rays and facet_geometry add the files they add to make_scene.  With
    scan_file the cleaned scan is written there (points, normals, sensor_position).  Returns the stages' results: dict of "scan" (clean_scan's
    dict), "triangulation", "features"."""
    from .scene_features import build_scene_features
    from .triangulate import triangulate_scan

    folder = os.path.dirname(out_base)
    if folder:
        os.makedirs(folder, exist_ok=True)
    if clean:
        scan = clean_scan(points, sensor_position, device=device, **clean_args)
    else:
        if clean_args:
            raise ValueError("scene_from_scan: %s given with clean=False" % ", ".join(sorted(clean_args)))
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        scan = dict(points=p, sensor_position=np.ascontiguousarray(sensor_position, dtype=np.float64).reshape(-1, 3), normals=None,
                    kept=np.arange(len(p), dtype=np.int64), stats=None)
    if scan_file is not None:
        if scan["normals"] is None:
            raise ValueError("scene_from_scan: scan_file needs the normals of a cleaned scan (clean=True)")
        np.savez(scan_file, points=scan["points"], normals=scan["normals"], sensor_position=scan["sensor_position"])
    tri = triangulate_scan(scan["points"], out_base=out_base, device=device)
    feat = build_scene_features(tri["mdata"], tri["infinite"], scan["points"], scan["sensor_position"], out_base=out_base, device=device,
                                facet_rays=facet_rays, facet_geometry=facet_geometry)
    np.savez(out_base + "_labels.npz", infinite=tri["infinite"])
    return dict(scan=scan, triangulation=tri, features=feat)
