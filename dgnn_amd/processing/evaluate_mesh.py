"""Scores any triangle mesh against the evaluation files of a scene on the device: the reference's `iou` and `chamfer`
(processing/generate_mesh.py:126-163, processing/evaluate_mesh.py) for a mesh that did not come from this library's labelled
tetrahedralization -- a baseline method's output, a mesh read with sample_mesh.read_off."""
from __future__ import annotations

import numpy as np
import torch


def evaluate(vertices, faces, occ_file=None, pointcloud_file=None, seed=0, device=None, topology=False) -> dict:
    """-> {"iou": ..., "chamfer": ...}, each present when its file is given; with `topology` also "components", "largest_component_faces"
    and "watertight".
    iou      check_mesh_contains of the mesh at the points of `occ_file` (points.npz) against its occupancies, compute_iou's ratio
             (ops.mesh_occupancy_iou);
    chamfer  as many points as `pointcloud_file` (pointcloud.npz) holds, sampled on the faces by area with `seed` (ops.sample_interface),
             against its points, exact nearest neighbours both ways (ops.chamfer_distance); inf with a warning for a mesh without faces.
    components, largest_component_faces  the number of connected components (faces connected through shared edges, ops.mesh_components)
             and the face count of the largest one (ops.mesh_component_measures); 0 and 0 for a mesh without faces;
    watertight  ops.mesh_topology's (Open3D's is_watertight without the self-intersection test); 0 for a mesh without faces.
    For the mesh `generate` returns these are generate's numbers (`evaluation.occupancy: mesh`, `evaluation.seed`, `mesh.solver: gpu`)."""
    from ..ops import chamfer_distance, mesh_component_measures, mesh_components, mesh_occupancy_iou, mesh_topology, sample_interface
    from .generate_mesh import load_occupancy

    dev = torch.device(device or "cuda:0")
    v = torch.as_tensor(np.asarray(vertices, dtype=np.float64)).to(dev)
    f = torch.as_tensor(np.asarray(faces, dtype=np.int32).reshape(-1, 3)).to(dev)
    out = dict()
    if topology:
        comp, k = mesh_components(f, len(v))
        out["components"] = k
        out["largest_component_faces"] = int(mesh_component_measures(v, f, comp, k)["n_faces"].max().item()) if k else 0
        out["watertight"] = mesh_topology(f, len(v))["watertight"]
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
