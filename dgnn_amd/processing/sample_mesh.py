"""The evaluation samples of one ground-truth mesh (reference processing/<dataset>/sample_mesh.py: export_pointcloud :61-87 and
export_points :106-147), computed on the device: `pointcloud.npz` (points on the surface with their normals) and `points.npz` (points in
the padded box and near the surface with their occupancies), the two files every `iou` / `chamfer` metric reads.

The argument names and defaults are the reference's (`packbits` defaults to what its script sets before it runs: True); `seed` is new.
The random streams are this library's counter hash (include/dgnn_hip.h: mm_hash), not np.random: a file is reproducible from its seed,
and it is NOT the file the reference would draw.  The three streams of one seed are seed (surface samples of either file),
seed + 1 (box points) and seed + 2 (jitter).
"""
from __future__ import annotations

import os

import numpy as np
import torch


def read_off(path):
    """A plain OFF file -> (vertices fp64 [V, 3], faces int32 [F, 3]).  The `OFF` keyword may stand on its own line or run into the
    counts (`OFF8 12 0`, as some ModelNet files have it); `#` comments and blank lines are skipped; triangle faces only."""
    with open(path, "r") as fh:
        tok = []
        for line in fh:
            line = line.split("#", 1)[0].strip()
            if line:
                tok.extend(line.split())
    if not tok or not tok[0].upper().startswith("OFF"):
        raise ValueError("%s: not an OFF file" % path)
    tok = ([tok[0][3:]] if len(tok[0]) > 3 else []) + tok[1:]
    try:
        nv, nf = int(tok[0]), int(tok[1])
        vertices = np.array(tok[3:3 + 3 * nv], dtype=np.float64).reshape(nv, 3)
        rest = tok[3 + 3 * nv:]
        faces = np.empty((nf, 3), dtype=np.int32)
        k = 0
        for i in range(nf):
            if int(rest[k]) != 3:
                raise ValueError("%s: face %d has %s vertices; only triangles are read" % (path, i, rest[k]))
            faces[i] = [int(rest[k + 1]), int(rest[k + 2]), int(rest[k + 3])]
            k += 4          # colours after a face are not supported: the next token must be a count again
    except (IndexError, ValueError) as e:
        raise ValueError("%s: malformed OFF file (%s)" % (path, e)) from None
    return vertices, faces


def _dtype(float16):
    return np.float16 if float16 else np.float32


def _prepare(filename, overwrite, what):
    if not overwrite and os.path.exists(filename):
        print("%s already exist: %s" % (what, filename))
        return False
    os.makedirs(os.path.dirname(filename) or ".", exist_ok=True)
    return True


def write_points_file(filename, points, occupancies, loc=None, scale=75.0, float16=False, packbits=True):
    """points.npz as the reference lays it out (:134-147): points cast to fp32 / fp16, occupancies bool [n] bit-packed with packbits"""
    occupancies = np.asarray(occupancies, dtype=bool)
    if packbits:
        occupancies = np.packbits(occupancies)
    np.savez(filename, points=np.asarray(points).astype(_dtype(float16)), occupancies=occupancies, loc=np.zeros(3) if loc is None else np.asarray(loc),
             scale=scale)
    return filename


def export_pointcloud(vertices, faces, filename, pointcloud_size=100000, scale=75.0, loc=None, float16=False, overwrite=True, seed=0, device=None):
    """pointcloud.npz: `points` sampled on the faces by area (ops.sample_interface) and `normals`, the unit normals of their faces
    (ops.face_normals), both fp32 (fp16 with float16), with `loc` and `scale`.  -> the file name, None when it exists and is kept."""
    from ..ops import face_normals, sample_interface

    if not _prepare(filename, overwrite, "Pointcloud"):
        return None
    dev = torch.device(device or "cuda:0")
    v = torch.as_tensor(np.asarray(vertices, dtype=np.float64)).to(dev)
    f = torch.as_tensor(np.asarray(faces, dtype=np.int32)).to(dev)
    points, face_idx = sample_interface(v, f, None, pointcloud_size, seed=seed)
    normals = face_normals(v, f)[face_idx.long()]
    dtype = _dtype(float16)
    print("Writing pointcloud: %s" % filename)
    np.savez(filename, points=points.cpu().numpy().astype(dtype), normals=normals.cpu().numpy().astype(dtype),
             loc=np.zeros(3) if loc is None else np.asarray(loc), scale=scale)
    return filename


def sample_points(vertices, faces, points_size=100000, points_uniform_ratio=1., points_sigma=0.05, points_padding=0.75, scale=75.0, seed=0, device=None):
    """The fp64 query points of export_points on the device: int(points_size * points_uniform_ratio) uniform in the box of edge scale +
    points_padding about the origin (ops.box_points), the rest on the surface (ops.sample_interface) with N(0, points_sigma) added per
    coordinate (ops.jitter_points), in that order."""
    from ..ops import box_points, jitter_points, sample_interface

    dev = torch.device(device or "cuda:0")
    n_uniform = int(points_size * points_uniform_ratio)
    n_surface = points_size - n_uniform
    parts = [box_points(n_uniform, scale + points_padding, seed=seed + 1, device=dev)]
    if n_surface > 0:
        surf, _ = sample_interface(torch.as_tensor(np.asarray(vertices, dtype=np.float64)).to(dev), torch.as_tensor(np.asarray(faces, dtype=np.int32)).to(dev),
                                   None, n_surface, seed=seed)
        parts.append(jitter_points(surf.to(torch.float64), points_sigma, seed=seed + 2))
    return torch.cat(parts, dim=0)


def export_points(vertices, faces, filename, points_size=100000, points_uniform_ratio=1., points_sigma=0.05, points_padding=0.75, scale=75.0, loc=None,
                  float16=False, packbits=True, overwrite=True, seed=0, device=None, modelname=None):
    """points.npz: `points` (sample_points, stored fp32 / fp16) and their `occupancies` in the mesh, computed on the fp64 points BEFORE
    the cast as the reference does (ops.mesh_contains), bit-packed with packbits; `loc`, `scale`.  A mesh that is not watertight -- an
    edge that is not in exactly two faces (ops.mesh_topology) -- is refused with the reference's warning and nothing is written.
    -> the file name, or None."""
    from ..ops import mesh_contains, mesh_topology

    dev = torch.device(device or "cuda:0")
    f = torch.as_tensor(np.asarray(faces, dtype=np.int32)).to(dev)
    topo = mesh_topology(f, len(vertices)) if len(f) else None
    if topo is None or topo["boundary_edges"] or topo["nonmanifold_edges"]:
        print("Warning: mesh %s is not watertight!Cannot sample points." % (modelname if modelname is not None else filename))
        return None
    if not _prepare(filename, overwrite, "Points"):
        return None
    points = sample_points(vertices, faces, points_size, points_uniform_ratio, points_sigma, points_padding, scale, seed, dev)
    occupancies, n_disagree = mesh_contains(vertices, f, points)
    if n_disagree:
        print("Warning: contains1 != contains2 for some points.")
    print("Writing points: %s" % filename)
    return write_points_file(filename, points.cpu().numpy(), occupancies.cpu().numpy(), loc, scale, float16, packbits)


def sample_mesh(vertices, faces, out_dir, pointcloud_size=100000, points_size=100000, points_uniform_ratio=1., points_sigma=0.05, points_padding=0.75,
                scale=75.0, float16=False, packbits=True, overwrite=True, seed=0, device=None):
    """Both files of one mesh into out_dir (the reference's eval/<id>/): -> {"pointcloud": path or None, "points": path or None}"""
    return {"pointcloud": export_pointcloud(vertices, faces, os.path.join(out_dir, "pointcloud.npz"), pointcloud_size, scale, None, float16, overwrite, seed,
                                            device),
            "points": export_points(vertices, faces, os.path.join(out_dir, "points.npz"), points_size, points_uniform_ratio, points_sigma, points_padding,
                                    scale, None, float16, packbits, overwrite, seed, device, modelname=os.path.basename(os.path.normpath(out_dir)))}
