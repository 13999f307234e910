"""CPU model of the mesh `generate` returns with ``mesh.solver: gpu`` (the contract of dgnn_orient_interface / dgnn_compact_vertices /
dgnn_mesh_topology).  It shares no arithmetic with the device:

* orientation: the sign of det[b - a, c - a, p - a] from an fp64 evaluation where it clears a deliberately loose bound (1e-10 of the
  permanent), else from `fractions.Fraction` arithmetic on the exact coordinates; the rule of include/dgnn_hip.h on top;
* compaction: np.unique and a search;
* topology: edge and vertex counts from plain dictionaries, vertex fans by a breadth-first search per vertex (Open3D's IsVertexManifold);
* the signed volume of a closed, outward-wound surface about a point, against the volume of the inside cells.
Scenes and labels come from tests/mesh_metrics_model.py.
"""
from __future__ import annotations

from collections import defaultdict
from fractions import Fraction

import numpy as np

from mesh_metrics_model import interface_ids, orient  # noqa: F401  (interface_ids: re-exported for the tests)

LOOSE = 1e-10


def _permanent(a, b, c, p):
    u, v, w = b - a, c - a, p - a
    return (np.abs(u[..., 0]) * (np.abs(v[..., 1] * w[..., 2]) + np.abs(v[..., 2] * w[..., 1]))
            + np.abs(u[..., 1]) * (np.abs(v[..., 0] * w[..., 2]) + np.abs(v[..., 2] * w[..., 0]))
            + np.abs(u[..., 2]) * (np.abs(v[..., 0] * w[..., 1]) + np.abs(v[..., 1] * w[..., 0])))


def exact_det(a, b, c, p):
    """det[b - a, c - a, p - a] as a Fraction (one point each)"""
    a, b, c, p = ([Fraction(float(x)) for x in q] for q in (a, b, c, p))
    u = [b[i] - a[i] for i in range(3)]
    v = [c[i] - a[i] for i in range(3)]
    w = [p[i] - a[i] for i in range(3)]
    return u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0]) + u[2] * (v[0] * w[1] - v[1] * w[0])


def orient_sign(a, b, c, p, return_exact_rows=False):
    """exact sign (int8 [K]) of det[b - a, c - a, p - a] for [K, 3] arrays"""
    a, b, c, p = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (a, b, c, p))
    o = orient(a, b, c, p)
    sure = np.abs(o) > LOOSE * _permanent(a, b, c, p) + 1e-250
    s = np.sign(o).astype(np.int8)
    rows = np.nonzero(~sure)[0]
    for i in rows:
        d = exact_det(a[i], b[i], c[i], p[i])
        s[i] = (d > 0) - (d < 0)
    return (s, rows) if return_exact_rows else s


def naive_sign(a, b, c, p):
    """the plain fp64 sign (what the exact stage exists to correct)"""
    return np.sign(orient(*(np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (a, b, c, p)))).astype(np.int8)


def _opposite(tets, cells, facets):
    """the vertex of each cell that is not on its facet"""
    t = tets[cells]
    on = (t[:, :, None] == facets[:, None, :]).any(axis=2)
    assert (on.sum(axis=1) == 3).all()
    return t[~on]


def orient_interface(scene, labels, ids, fix=True):
    """-> (faces int32 [K, 3], n_undetermined): facets[ids] wound away from their inside cell (label 0; cell -1 outside)"""
    v, tets = scene["vertices"], np.asarray(scene["tetrahedra"], dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    fac = np.asarray(scene["facets"], dtype=np.int64)[ids]
    cells = np.asarray(scene["nfacets"], dtype=np.int64)[ids]
    if not fix or len(ids) == 0:
        return fac.astype(np.int32).reshape(-1, 3), 0
    lab = np.append(np.asarray(labels), 1)
    inside = lab[np.where(cells < 0, len(labels), cells)] == 0
    assert (inside.sum(axis=1) == 1).all()
    ci = np.where(inside[:, 0], cells[:, 0], cells[:, 1])
    co = np.where(inside[:, 0], cells[:, 1], cells[:, 0])
    a, b, c = v[fac[:, 0]], v[fac[:, 1]], v[fac[:, 2]]
    s = orient_sign(a, b, c, v[_opposite(tets, ci, fac)])
    flat = np.nonzero((s == 0) & (co >= 0))[0]
    if len(flat):
        s[flat] = -orient_sign(a[flat], b[flat], c[flat], v[_opposite(tets, co[flat], fac[flat])])
    out = fac.copy()
    swap = s > 0
    out[swap, 1], out[swap, 2] = fac[swap, 2], fac[swap, 1]
    return out.astype(np.int32), int((s == 0).sum())


def compact(faces):
    """-> (faces renumbered onto the kept vertices, kept ids ascending)"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    kept = np.unique(faces)
    return np.searchsorted(kept, faces).astype(np.int32), kept.astype(np.int32)


def topology(faces):
    """edge and vertex counts by dictionaries (keys as ops.MESH_TOPOLOGY_KEYS, + watertight)"""
    faces = [tuple(int(x) for x in f) for f in np.asarray(faces).reshape(-1, 3)]
    edge_faces = defaultdict(list)
    directed = defaultdict(int)
    vert_faces = defaultdict(list)
    for t, f in enumerate(faces):
        for k in range(3):
            u, w = f[k], f[(k + 1) % 3]
            edge_faces[(min(u, w), max(u, w))].append(t)
            directed[(u, w)] += 1
            vert_faces[f[k]].append(t)
    n_faces = {e: len(ts) for e, ts in edge_faces.items()}
    nonmanifold_vertices = 0
    for v, ts in vert_faces.items():            # Open3D's IsVertexManifold: the faces at v connected through edges that contain v
        seen = {ts[0]}
        queue = [ts[0]]
        while queue:
            t = queue.pop()
            for nb in faces[t]:
                if nb == v:
                    continue
                for t2 in edge_faces[(min(v, nb), max(v, nb))]:
                    if t2 not in seen:
                        seen.add(t2)
                        queue.append(t2)
        nonmanifold_vertices += len(seen) != len(set(ts))
    out = dict(n_edges=len(n_faces), boundary_edges=sum(n == 1 for n in n_faces.values()),
               nonmanifold_edges=sum(n >= 3 for n in n_faces.values()), nonmanifold_vertices=nonmanifold_vertices,
               winding_mismatch_edges=sum(directed[(u, w)] != directed[(w, u)] for (u, w) in n_faces))
    out["watertight"] = int(len(faces) > 0 and out["boundary_edges"] == 0 and out["nonmanifold_edges"] == 0 and out["nonmanifold_vertices"] == 0)
    return out


def signed_volume(vertices, faces, about=None):
    """sum over the faces of det[a - o, b - o, c - o] / 6 (o = `about`, default the vertices' centroid)"""
    v = np.asarray(vertices, dtype=np.float64)
    o = v.mean(axis=0) if about is None else np.asarray(about, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]] - o, v[f[:, 1]] - o, v[f[:, 2]] - o
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def inside_volume(scene, labels):
    v, t = scene["vertices"], np.asarray(scene["tetrahedra"], dtype=np.int64)
    t = t[np.asarray(labels) == 0]
    a = v[t[:, 0]]
    return float(np.abs(np.einsum("ij,ij->i", v[t[:, 1]] - a, np.cross(v[t[:, 2]] - a, v[t[:, 3]] - a))).sum() / 6.0)


# ---- hand-made scenes ------------------------------------------------------------------------------------------------------------
def tetra_faces(t):
    """the four faces of tetrahedron t (4 vertex ids), wound outward when t is positively oriented"""
    a, b, c, d = t
    return [(a, c, b), (a, b, d), (a, d, c), (b, c, d)]


def regular_grid_scene(n=10, seed=0, scale=7.3, offset=(0.31, -2.7, 5.1)):
    """scipy's Delaunay of an n^3 grid (many flat cells), then the vertices randomly rotated, scaled and shifted: the flat cells become
    nearly flat, with signs that plain fp64 gets wrong"""
    from mesh_metrics_model import scene_from_points

    g = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    scene = scene_from_points(g)
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    scene["vertices"] = g @ q.T * scale + np.asarray(offset)
    return scene
