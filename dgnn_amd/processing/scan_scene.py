"""From a raw scan to a scene folder: what a user with points and sensor positions, and no ground-truth mesh, starts from -- the
arrays of the reference's `scan/<name>.npz` (processing/reconbench/ply2npz.py, processing/eth3d/feat.py).

subsample_scan thins a dense scan first (one point per voxel, ops.voxel_subsample, then no two points closer than a radius,
ops.min_distance_thin); clean_scan removes the statistical outliers (ops.outlier_mask) and estimates the normals the reference's scan files
carry (ops.estimate_normals, turned towards each point's sensor); scene_from_scan chains them with triangulate_scan and build_scene_features and writes the `_labels.npz` the
loader opens.  A scan has no labels: that file holds `infinite` alone, which is all dataLoader.run reads of it with inference.has_label off; a
training run on such a folder fails on the missing key.  make_scene (a scene from a ground-truth mesh) is in triangulate.py.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import ops


def _scan_arrays(points, sensor_position, what):
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    s = np.ascontiguousarray(sensor_position, dtype=np.float64).reshape(-1, 3)
    if len(p) != len(s):
        raise ValueError("%s: %d sensor positions for %d points" % (what, len(s), len(p)))
    return p, s


def subsample_scan(points, sensor_position, voxel_size=None, representative="nearest", min_distance=None, seed=0, device=None):
    """points, sensor_position [P, 3] -> dict: "points", "sensor_position" fp64 of the kept rows, in ascending input index; "kept" int64: their
    input rows; "stats".  With voxel_size one point per occupied voxel of that edge (origin 0) stays: the member nearest the voxel's centroid
    (representative="nearest") or its lowest member ("first") -- an input point either way, which keeps its own sensor position.  With
    min_distance what is left is thinned so that no two kept points are closer (ops.min_distance_thin in the hashed order of `seed`, the rows
    counted among what the voxel step left).  The voxel step comes first: it is one sort whatever the density, and hands the thinning the even
    density whose conflict lists are short.  stats: n_in, n_out, and voxels (the occupied voxels) / thinning (ops.min_distance_thin's stats) for
    the steps taken."""
    if representative not in ("nearest", "first"):
        raise ValueError("subsample_scan: representative=%r, expected 'nearest' or 'first'" % (representative,))
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    p, s = _scan_arrays(points, sensor_position, "subsample_scan")
    kept = np.arange(len(p), dtype=np.int64)
    stats = dict(n_in=len(p))
    if voxel_size is not None or min_distance is not None:
        dp = torch.from_numpy(p).to(dev)
        if voxel_size is not None:
            vox = ops.voxel_subsample(dp, voxel_size)
            kept = torch.sort(vox[representative].long()).values          # one member per voxel: unique
            stats["voxels"] = vox["m"]
            dp = dp[kept].contiguous()
            kept = kept.cpu().numpy()
        if min_distance is not None:
            keep, stats["thinning"] = ops.min_distance_thin(dp, min_distance, seed=seed, return_stats=True)
            kept = kept[np.nonzero(keep.cpu().numpy())[0]]
    stats["n_out"] = len(kept)
    return dict(points=p[kept], sensor_position=s[kept], kept=kept, stats=stats)


def clean_scan(points, sensor_position, outlier_k=16, std_ratio=2.0, normals_k=16, device=None):
    """points, sensor_position [P, 3] -> dict: "points", "sensor_position", "normals" fp64 of the kept points, in input order; "kept" int64: their
    input rows; "stats": those of ops.outlier_mask with mean_distance on the host (None when std_ratio is None: nothing is removed)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    p, s = _scan_arrays(points, sensor_position, "clean_scan")
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


def scene_from_scan(points, sensor_position, out_base, clean=True, facet_rays=False, facet_geometry=False, scan_file=None, device=None,
                    voxel_size=None, min_distance=None, seed=0, **clean_args):
    """A raw scan -> every file dataLoader.run opens with inference.has_label off: subsample_scan(voxel_size, min_distance, seed) when either
    is given (BEFORE the cleaning: the outlier statistic is a density statistic and should see the even density) -> clean_scan(**clean_args)
    (clean=False: the scan as it is, no normals) -> triangulate_scan -> build_scene_features, written as out_base + "_3dt.npz",
    "_adjacencies.npz", "_cgeom.npz", "_cbvf.npz", "_fbvf.npz" and "_labels.npz" (the key `infinite` only); facet_rays and facet_geometry add the files they add to make_scene.  With
    scan_file the cleaned scan is written there (points, normals, sensor_position).  Returns the stages' results: dict of "scan" (clean_scan's
    dict; its "kept" are rows of the INPUT, both selections composed, and with a subsampling step its stats are under "subsample"),
    "triangulation", "features"."""
    from .scene_features import build_scene_features
    from .triangulate import triangulate_scan

    folder = os.path.dirname(out_base)
    if folder:
        os.makedirs(folder, exist_ok=True)
    sub = None
    if voxel_size is not None or min_distance is not None:
        sub = subsample_scan(points, sensor_position, voxel_size=voxel_size, min_distance=min_distance, seed=seed, device=device)
        points, sensor_position = sub["points"], sub["sensor_position"]
    if clean:
        scan = clean_scan(points, sensor_position, device=device, **clean_args)
    else:
        if clean_args:
            raise ValueError("scene_from_scan: %s given with clean=False" % ", ".join(sorted(clean_args)))
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        scan = dict(points=p, sensor_position=np.ascontiguousarray(sensor_position, dtype=np.float64).reshape(-1, 3), normals=None,
                    kept=np.arange(len(p), dtype=np.int64), stats=None)
    if sub is not None:
        scan = dict(scan, kept=sub["kept"][scan["kept"]], subsample=sub["stats"])
    if scan_file is not None:
        if scan["normals"] is None:
            raise ValueError("scene_from_scan: scan_file needs the normals of a cleaned scan (clean=True)")
        np.savez(scan_file, points=scan["points"], normals=scan["normals"], sensor_position=scan["sensor_position"])
    tri = triangulate_scan(scan["points"], out_base=out_base, device=device)
    feat = build_scene_features(tri["mdata"], tri["infinite"], scan["points"], scan["sensor_position"], out_base=out_base, device=device,
                                facet_rays=facet_rays, facet_geometry=facet_geometry)
    np.savez(out_base + "_labels.npz", infinite=tri["infinite"])
    return dict(scan=scan, triangulation=tri, features=feat)
