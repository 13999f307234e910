"""Scores any triangle mesh against the evaluation files of a scene on the device: the reference's `iou` and `chamfer`
(processing/generate_mesh.py:126-163, processing/evaluate_mesh.py) for a mesh that did not come from this library's labelled
tetrahedralization -- a baseline method's output, a mesh read with sample_mesh.read_off."""
from __future__ import annotations

import numpy as np
import torch


DEFAULT_FSCORE_THRESHOLDS = (0.01, 0.02)          # ConvONet's F-score columns for shapes normalised to the unit cube: a convention, not a measurement


def pointcloud_metrics(vertices, faces, gt_points, gt_normals=None, thresholds=DEFAULT_FSCORE_THRESHOLDS, seed=0, name=""):
    """The surface metrics of a mesh (vertices fp64 [V, 3], faces int32 [F, 3], on the GPU) against a ground-truth POINT CLOUD with normals
    (pointcloud.npz's `points` and `normals`) -- the normal consistency the reference leaves as a TODO (processing/generate_mesh.py:154):
    completeness / recall  every ground-truth point to the MESH (ops.point_mesh_distance), its cosine between the point's normal and the
                           closest face's normal;
    accuracy / precision   len(gt_points) samples of the mesh by area (ops.sample_interface, `seed`) to the ground-truth points
                           (ops.nearest_neighbor: fp32, exact), the cosine between the sample's face normal and the nearest point's normal.
    -> dict of the keys of ops.surface_metric_values (normal_consistency only with gt_normals).  A mesh without faces or area, or an empty
    cloud, gives inf distances and zero scores with a warning; any other failure raises."""
    from .. import ops

    thresholds = [float(t) for t in thresholds]
    dev = vertices.device
    gt = torch.as_tensor(np.asarray(gt_points, dtype=np.float32).reshape(-1, 3)).to(dev)
    nrm = None if gt_normals is None else torch.as_tensor(np.asarray(gt_normals, dtype=np.float64).reshape(-1, 3)).to(dev)
    n = len(gt)
    if len(faces) == 0 or n == 0:
        print("WARNING: Mesh {} has no faces or its ground truth no points; surface distances set to inf and scores to 0".format(name))
        return ops.empty_surface_metrics(thresholds, nrm is not None)
    fn = ops.face_normals(vertices, faces)
    if not bool(fn.any()):          # every normal zero: no face has area, nothing to sample
        print("WARNING: Mesh {} has no area to sample; surface distances set to inf and scores to 0".format(name))
        return ops.empty_surface_metrics(thresholds, nrm is not None)
    recon, recon_face = ops.sample_interface(vertices, faces, None, n, seed=seed)
    d_gt, f_gt, _, _ = ops.point_mesh_distance(vertices, faces, gt)
    d_rc, i_rc, _ = ops.nearest_neighbor(gt, recon)
    c_gt = c_rc = None
    if nrm is not None:
        ids = torch.arange(n, dtype=torch.int32, device=dev)
        c_gt, c_rc = ops.row_dot3(nrm, ids, fn, f_gt), ops.row_dot3(fn, recon_face, nrm, i_rc)
    return ops.surface_metric_values(ops.distance_fold(d_rc, c_rc, thresholds), n, ops.distance_fold(d_gt, c_gt, thresholds), n, thresholds, nrm is not None)


def evaluate(vertices, faces, occ_file=None, pointcloud_file=None, seed=0, device=None, topology=False, gt_mesh=None,
             thresholds=DEFAULT_FSCORE_THRESHOLDS, n_samples=100000, surface_metrics=False) -> dict:
    """-> {"iou": ..., "chamfer": ...}, each present when its file is given; with `topology` also "components", "largest_component_faces"
    and "watertight"; with `gt_mesh` or `surface_metrics` also the surface metrics below.
    iou      check_mesh_contains of the mesh at the points of `occ_file` (points.npz) against its occupancies, compute_iou's ratio
             (ops.mesh_occupancy_iou);
    chamfer  as many points as `pointcloud_file` (pointcloud.npz) holds, sampled on the faces by area with `seed` (ops.sample_interface),
             against its points, exact nearest neighbours both ways (ops.chamfer_distance); inf with a warning for a mesh without faces.
    components, largest_component_faces  the number of connected components (faces connected through shared edges, ops.mesh_components)
             and the face count of the largest one (ops.mesh_component_measures); 0 and 0 for a mesh without faces;
    watertight  ops.mesh_topology's (Open3D's is_watertight without the self-intersection test); 0 for a mesh without faces.
    gt_mesh=(vertices, faces)  adds the keys of ops.surface_metrics, the evaluated mesh as A and the ground-truth mesh as B, `n_samples` per side
             with `seed` / `seed + 1`: "accuracy", "completeness", "chamfer_mesh", "hausdorff", "normal_consistency" and, per threshold t of
             `thresholds`, "precision@t", "recall@t", "fscore@t";
    surface_metrics=True  with `pointcloud_file`: the same keys against the file's `points` and `normals` (pointcloud_metrics; without
             `normals` in the file there is no "normal_consistency").  gt_mesh wins when both are given.
    For the mesh `generate` returns these are generate's numbers (`evaluation.occupancy: mesh`, `evaluation.seed`, `mesh.solver: gpu`,
    `evaluation.fscore_thresholds`)."""
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
    if gt_mesh is not None:
        from ..ops import surface_metrics as mesh_surface_metrics

        gv = torch.as_tensor(np.asarray(gt_mesh[0], dtype=np.float64)).to(dev)
        gf = torch.as_tensor(np.asarray(gt_mesh[1], dtype=np.int32).reshape(-1, 3)).to(dev)
        out.update(mesh_surface_metrics(v, f, gv, gf, n_samples, thresholds, seed=seed))
    elif surface_metrics:
        if pointcloud_file is None:
            raise ValueError("evaluate: surface_metrics needs gt_mesh or pointcloud_file")
        cloud = np.load(pointcloud_file)
        out.update(pointcloud_metrics(v, f, cloud["points"], cloud["normals"] if "normals" in cloud else None, thresholds, seed=seed))
    return out
