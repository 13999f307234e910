"""Scores any triangle mesh against the evaluation files of a scene on the device: the reference's `iou` and `chamfer`
(processing/generate_mesh.py:126-163, processing/evaluate_mesh.py) for a mesh that did not come from this library's labelled
tetrahedralization -- a baseline method's output, a mesh read with sample_mesh.read_off."""
from __future__ import annotations

import numpy as np
import torch


def evaluate(vertices, faces, occ_file=None, pointcloud_file=None, seed=0, device=None) -> dict:
    """-> {"iou": ..., "chamfer": ...}, each present when its file is given.
    iou      check_mesh_contains of the mesh at the points of `occ_file` (points.npz) against its occupancies, compute_iou's ratio
             (ops.mesh_occupancy_iou);
    chamfer  as many points as `pointcloud_file` (pointcloud.npz) holds, sampled on the faces by area with `seed` (ops.sample_interface),
             against its points, exact nearest neighbours both ways (ops.chamfer_distance); inf with a warning for a mesh without faces.
    For the mesh `generate` returns these are generate's numbers (`evaluation.occupancy: mesh`, `evaluation.seed`)."""
    from ..ops import chamfer_distance, mesh_occupancy_iou, sample_interface
    from .generate_mesh import load_occupancy

    dev = torch.device(device or "cuda:0")
    v = torch.as_tensor(np.asarray(vertices, dtype=np.float64)).to(dev)
    f = torch.as_tensor(np.asarray(faces, dtype=np.int32).reshape(-1, 3)).to(dev)
    out = dict()
    if occ_file is not None:
        points, gt = load_occupancy(occ_file)
        out["iou"] = mesh_occupancy_iou(v, f, torch.from_numpy(points).to(dev), gt)[0]
    if pointcloud_file is not None:
        gt_points = np.load(pointcloud_file)["points"].astype(np.float32)
        if len(f) == 0:
            print("WARNING: the mesh has no faces; Chamfer distance set to inf")
            out["chamfer"] = float("inf")
        else:
            recon, _ = sample_interface(v, f, None, len(gt_points), seed=seed)
            out["chamfer"] = chamfer_distance(torch.from_numpy(gt_points).to(dev), recon)
    return out
