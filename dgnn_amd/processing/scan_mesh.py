"""A virtual scanner: a closed mesh becomes the scan the pipeline starts from -- points, normals and sensor positions.

The reference makes every ModelNet and ShapeNet training scene with an external `scan` binary (processing/modelnet/scan.py:61-72,
processing/shapenet/scan.py:50-74: `--points --cameras --noise --outliers`) and keeps `points`, `normals`, `gt_normals` and
`sensor_position`.  That binary's generator is not known: what follows is THIS PACKAGE'S DEFINITION of a scan, not a reproduction of its
output.  The arrays are the ones build_scene_features (scan_points, sensor_position) and the reference's loaders read, so the chain is
mesh -> scan_mesh -> (a triangulator) -> build_scene_features / build_cell_labels.

Cameras sit on a sphere about the mesh; every ray starts at a camera and aims at an area-uniform sample of the surface; the scan point is
the FIRST face the ray meets (ops.ray_first_hit, exact crossing signs), so an aim that another part of the surface hides yields the nearer
surface.  Randomness is the library's counter hash (include/dgnn_hip.h: mm_hash): a scan is reproducible from its seed.  The five streams
of one seed are mm_hash(seed, 1..5): aims, sensor choice, noise, outlier positions, outlier sensors.
"""
from __future__ import annotations

import os

import numpy as np
import torch

SCAN_KEYS = ("points", "normals", "gt_normals", "sensor_position", "cameras", "noise", "outliers")          # shapenet/scan.py:67-74
SCAN_STATS = ("rays", "hits", "misses", "other_face", "degenerate", "exact_used")
_M64 = 0xFFFFFFFFFFFFFFFF


def mm_hash(seed, ctr):
    """include/dgnn_hip.h mm_hash on uint64 arrays (wrapping), on the host"""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & _M64) + np.asarray(ctr, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _u01(h):
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _frame(vertices, faces):
    """(centre of the referenced vertices' box, half its diagonal), host fp64"""
    v, f = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        raise ValueError("scan_mesh: a mesh without faces")
    if f.min() < 0 or f.max() >= len(v):
        raise ValueError("scan_mesh: a face's vertex id out of range")
    used = v[np.unique(f)]
    lo, hi = used.min(axis=0), used.max(axis=0)
    ext = hi - lo
    return 0.5 * (lo + hi), 0.5 * np.sqrt((ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2])


def camera_positions(vertices, faces, n_cameras, distance=2.0, seed=0):
    """n_cameras sensor positions fp64 [n, 3] on the sphere of radius distance * radius about centre (the centre and half diagonal of the
    referenced vertices' box), uniform by area: camera k at centre + distance * radius * (sqrt(1 - z z) cos phi, sqrt(1 - z z) sin phi, z)
    with z = 2 u01(mm_hash(seed, 2 k + 1)) - 1 and phi = 2 pi u01(mm_hash(seed, 2 k + 2)).  Host numpy."""
    centre, radius = _frame(vertices, faces)
    k = np.arange(int(n_cameras), dtype=np.uint64)
    z = 2.0 * _u01(mm_hash(seed, np.uint64(2) * k + np.uint64(1))) - 1.0
    phi = 6.283185307179586 * _u01(mm_hash(seed, np.uint64(2) * k + np.uint64(2)))
    rho = np.sqrt(1.0 - z * z)
    unit = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)
    return centre + (float(distance) * radius) * unit


def _sensor_ids(seed, n, n_cameras):
    return (mm_hash(seed, np.arange(1, n + 1, dtype=np.uint64)) % np.uint64(n_cameras)).astype(np.int64)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def scan_mesh(vertices, faces, points=3000, cameras=10, noise=0.0, outliers=0.0, seed=0, camera_distance=2.0, sensors=None, device=None):
    """Scans the mesh (vertices [V, 3], faces int [F, 3]) with `points` rays from `cameras` cameras (camera_positions at camera_distance;
    `sensors` [C, 3] overrides them) on `device` (default: the current GPU):
      1. aims: ops.sample_interface(vertices, faces, None, points), area-uniform fp32 samples, cast to fp64;
      2. the sensor of ray i is camera mm_hash(s2, i + 1) mod C;
      3. ops.ray_first_hit; the hits, in ray order, are the scan points (the hit, not the aim);
      4. gt_normals: ops.face_normals of the hit face; normals: the same, negated where its dot with sensor - point is negative;
      5. noise > 0: ops.jitter_points(points, noise);
      6. outliers > 0: round(outliers * hits) more points, uniform in the cube of edge 2 radius about centre (ops.box_points), each with a
         camera of its own as sensor, the unit vector to it as `normals` and zeros as `gt_normals`.
    -> dict of fp64 ndarrays "points", "normals", "gt_normals", "sensor_position" [n, 3], "cameras" [C, 3] (the positions), "hit_face" int32
    (-1 for an outlier) and "stats": rays cast, hits, misses, hits on a face other than the aim's, degenerate crossings, exact-stage count."""
    from .. import ops

    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    centre, radius = _frame(vertices, faces)
    cams = camera_positions(vertices, faces, cameras, camera_distance, seed) if sensors is None else np.asarray(sensors, dtype=np.float64).reshape(-1, 3)
    if len(cams) == 0:
        raise ValueError("scan_mesh: no cameras")
    s1, s2, s3, s4, s5 = (int(x) for x in mm_hash(seed, np.arange(1, 6, dtype=np.uint64)))
    n = int(points)
    v = torch.from_numpy(np.ascontiguousarray(vertices, dtype=np.float64)).to(dev)
    f = torch.as_tensor(np.asarray(faces)).to(dev, torch.int32)
    cams_dev = torch.from_numpy(cams).to(dev)
    aims, aim_face = ops.sample_interface(v, f, None, n, seed=s1)
    origins = cams_dev[torch.from_numpy(_sensor_ids(s2, n, len(cams))).to(dev)]
    face, _, point, st = ops.ray_first_hit(v, f, origins, aims.to(torch.float64), return_stats=True)
    hit = face >= 0
    pts, sens, hit_face = point[hit], origins[hit], face[hit]
    gt = ops.face_normals(v, f)[hit_face.long()]
    flip = _dot(gt, sens - pts) < 0
    normals = torch.where(flip[:, None], -gt, gt)
    stats = dict(rays=n, hits=int(hit.sum()), misses=int((~hit).sum()), other_face=int((hit_face != aim_face[hit]).sum()), degenerate=st["degenerate"],
                 exact_used=st["exact_used"])
    if noise > 0:
        pts = ops.jitter_points(pts, noise, seed=s3)
    n_out = int(round(outliers * stats["hits"])) if outliers > 0 else 0
    if n_out:
        extra = ops.box_points(n_out, 2.0 * radius, seed=s4, device=dev) + torch.from_numpy(centre).to(dev)
        extra_sens = cams_dev[torch.from_numpy(_sensor_ids(s5, n_out, len(cams))).to(dev)]
        e = extra_sens - extra
        pts, sens = torch.cat([pts, extra]), torch.cat([sens, extra_sens])
        normals, gt = torch.cat([normals, e / torch.sqrt(_dot(e, e))[:, None]]), torch.cat([gt, torch.zeros_like(extra)])
        hit_face = torch.cat([hit_face, torch.full((n_out,), -1, dtype=torch.int32, device=dev)])
    host = lambda t: t.cpu().numpy()
    return {"points": host(pts), "normals": host(normals), "gt_normals": host(gt), "sensor_position": host(sens), "cameras": cams, "hit_face": host(hit_face),
            "stats": stats}


def export_scan(vertices, faces, filename, points=3000, cameras=10, noise=0.0, outliers=0.0, seed=0, camera_distance=2.0, sensors=None, device=None):
    """scan_mesh written as the reference keeps a scan (processing/shapenet/scan.py:67-74): points, normals, gt_normals, sensor_position [n, 3]
    and the scalars cameras (their number), noise, outliers, all fp64, in this key order.  -> the dict of scan_mesh."""
    scan = scan_mesh(vertices, faces, points, cameras, noise, outliers, seed, camera_distance, sensors, device)
    os.makedirs(os.path.dirname(filename) or ".", exist_ok=True)
    np.savez(filename, points=scan["points"], normals=scan["normals"], gt_normals=scan["gt_normals"], sensor_position=scan["sensor_position"],
             cameras=np.array(len(scan["cameras"]), dtype=np.float64), noise=np.array(noise, dtype=np.float64), outliers=np.array(outliers, dtype=np.float64))
    return scan
