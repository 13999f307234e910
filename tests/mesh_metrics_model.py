"""CPU model of the mesh metrics (the contract of dgnn_locate_points / dgnn_mesh_iou_counts / dgnn_sample_faces / dgnn_nearest_neighbor).

* scenes: seeded scipy Delaunay tetrahedralizations in `_3dt.npz` layout (vertices fp64, tetrahedra = finite cells, facets = vertex
  triples, nfacets = the two cells of each facet, -1 = the infinite cell), labelled by a sphere's signed distance at the centroids;
* containment: the reference's definition, ray parity against the interface triangles (check_mesh_contains), restated in fp64 for
  rays that stay clear of edges; and the same orientation arithmetic as the device walk (orient, cell_signs);
* sampler: mm_hash and the barycentric map of include/dgnn_hip.h, given the cumulative areas;
* nearest neighbour: fp32 brute force with the device's expression and tie rule; compute_chamfer with cKDTree.
"""
from __future__ import annotations

import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def scene_from_points(pts):
    """-> dict(vertices, tetrahedra, facets, nfacets) of scipy's Delaunay of `pts` (every facet once)"""
    from scipy.spatial import Delaunay

    pts = np.asarray(pts, dtype=np.float64)
    tri = Delaunay(pts)
    simp = tri.simplices.astype(np.int64)
    nbr = tri.neighbors.astype(np.int64)
    n = len(simp)
    c, k = np.nonzero((nbr < 0) | (nbr > np.arange(n)[:, None]))       # each facet from its lower cell (hull facets once)
    keep = np.ones((len(c), 4), dtype=bool)
    keep[np.arange(len(c)), k] = False
    facets = simp[c][keep].reshape(-1, 3)
    nfacets = np.stack([c, nbr[c, k]], axis=1)
    return dict(vertices=pts, tetrahedra=simp.astype(np.int32), facets=facets.astype(np.int32), nfacets=nfacets.astype(np.int32))


def random_scene(n_points, seed=0):
    return scene_from_points(np.random.default_rng(seed).random((n_points, 3)))


def centroids(scene):
    return scene["vertices"][scene["tetrahedra"]].mean(axis=1)


def sphere_labels(scene, center=0.5, radius=0.3):
    """0 = inside (centroid within the sphere), 1 = outside"""
    return (np.linalg.norm(centroids(scene) - center, axis=1) > radius).astype(np.int32)


def interface_ids(labels, nfacets):
    """facets between inside and outside cells, the infinite cell outside (generate_mesh.py:93-105)"""
    lab = np.append(np.asarray(labels), 1)
    cells = np.where(nfacets < 0, len(labels), nfacets)
    return np.nonzero(lab[cells[:, 0]] != lab[cells[:, 1]])[0].astype(np.int32)


# ---- containment -----------------------------------------------------------------------------------------------------------------
def orient(a, b, c, p):
    """det[b - a, c - a, p - a] with the device's operation order (fp64, no contraction)"""
    ux, uy, uz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
    vx, vy, vz = c[..., 0] - a[..., 0], c[..., 1] - a[..., 1], c[..., 2] - a[..., 2]
    wx, wy, wz = p[..., 0] - a[..., 0], p[..., 1] - a[..., 1], p[..., 2] - a[..., 2]
    return ux * (vy * wz - vz * wy) - uy * (vx * wz - vz * wx) + uz * (vx * wy - vy * wx)


def cell_signs(scene, cells, points):
    """[P, 4] bool: point on the side of vertex k of its cell (or on face k), by the device's rule (sorted facet ids; a flat cell holds
    only points on its plane)"""
    v, t = scene["vertices"], scene["tetrahedra"][cells].astype(np.int64)
    q = np.asarray(points, dtype=np.float32).astype(np.float64)
    ok = np.empty((len(cells), 4), dtype=bool)
    for k in range(4):
        f = np.sort(t[:, [(k + 1) % 4, (k + 2) % 4, (k + 3) % 4]], axis=1)
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        o, s = orient(a, b, c, q), orient(a, b, c, v[t[:, k]])
        ok[:, k] = np.where(s > 0, o >= 0, np.where(s < 0, o <= 0, o == 0))
    return ok


def brute_containing(scene, points):
    """[P, N] bool: every cell whose four signs are >= 0 (tiny scenes)"""
    n = len(scene["tetrahedra"])
    P = len(points)
    cells = np.tile(np.arange(n), P)
    pts = np.repeat(np.asarray(points, dtype=np.float32), n, axis=0)
    return cell_signs(scene, cells, pts).all(axis=1).reshape(P, n)


def ray_parity_inside(vertices, tris, points, direction=(0.5773, 0.5779, 0.5767), clear=1e-7):
    """check_mesh_contains' definition in fp64: a point is inside iff a ray from it crosses the triangles an odd number of times.
    -> (inside bool [P], clean bool [P]: no barycentric coordinate of a hit, and no ray parameter, within `clear` of 0)"""
    v = np.asarray(vertices, dtype=np.float64)
    tri = v[np.asarray(tris, dtype=np.int64)]
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    h = np.cross(d, e2)
    det = np.einsum("ij,ij->i", e1, h)
    inside = np.zeros(len(points), dtype=bool)
    clean = np.ones(len(points), dtype=bool)
    good = np.abs(det) > 1e-300
    for i, p in enumerate(np.asarray(points, dtype=np.float32).astype(np.float64)):
        s = p - a
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.einsum("ij,ij->i", s, h) / det
            qv = np.cross(s, e1)
            w = (qv @ d) / det
            t = np.einsum("ij,ij->i", e2, qv) / det
        near = good & (np.minimum.reduce([np.abs(u), np.abs(w), np.abs(1 - u - w)]) < clear) & (t > -clear)
        near |= good & (np.abs(t) < clear) & (u > -clear) & (w > -clear) & (u + w < 1 + clear)
        hit = good & (u > 0) & (w > 0) & (u + w < 1) & (t > 0)
        inside[i] = bool(hit.sum() & 1)
        clean[i] = not near.any()
    return inside, clean


def find_simplex_occupancy(points, scene_points, labels):
    """"label of Delaunay.find_simplex": inside iff the containing simplex is labelled 0 (outside the hull: outside)"""
    from scipy.spatial import Delaunay

    s = Delaunay(np.asarray(scene_points, dtype=np.float64)).find_simplex(np.asarray(points, dtype=np.float32).astype(np.float64))
    return (s >= 0) & (np.asarray(labels)[np.maximum(s, 0)] == 0)


def iou(occ, gt):
    """compute_iou (processing/evaluate_mesh.py): float32 counts and ratio"""
    occ1, occ2 = np.asarray(occ) >= 0.5, np.asarray(gt) >= 0.5
    with np.errstate(invalid="ignore", divide="ignore"):
        return float((occ1 & occ2).astype(np.float32).sum() / (occ1 | occ2).astype(np.float32).sum())


# ---- sampler ---------------------------------------------------------------------------------------------------------------------
def mm_hash(seed, ctr):
    """include/dgnn_hip.h mm_hash on uint64 arrays (wrapping)"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.asarray(ctr, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def face_areas(vertices, facets, face_ids):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(facets, dtype=np.int64)[np.asarray(face_ids, dtype=np.int64)]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = b - a, c - a
    cx, cy, cz = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return 0.5 * np.sqrt(cx * cx + cy * cy + cz * cz)


def sample(vertices, facets, face_ids, cum, n, seed):
    """-> (points fp32 [n, 3], face position int32 [n]) given the cumulative areas `cum`"""
    ctr = 3 * np.arange(n, dtype=np.uint64) + np.uint64(1)
    r0 = ((mm_hash(seed, ctr) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u = (mm_hash(seed, ctr + np.uint64(1)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    w = (mm_hash(seed, ctr + np.uint64(2)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    j = np.searchsorted(cum, r0 * cum[-1], side="left")
    flip = u + w > 1.0
    u = np.where(flip, 1.0 - u, u)
    w = np.where(flip, 1.0 - w, w)
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(facets, dtype=np.int64)[np.asarray(face_ids, dtype=np.int64)[j]]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    p = (u[:, None] * (b - a) + w[:, None] * (c - a)) + a
    return p.astype(np.float32), j.astype(np.int32)


# ---- nearest neighbour -----------------------------------------------------------------------------------------------------------
def nn_brute(ref, query, chunk=256):
    """fp32 (dx*dx + dy*dy) + dz*dz, ties to the smaller index -> (dist fp32, index int32)"""
    ref = np.asarray(ref, dtype=np.float32)
    query = np.asarray(query, dtype=np.float32)
    dist = np.empty(len(query), dtype=np.float32)
    idx = np.empty(len(query), dtype=np.int32)
    for s in range(0, len(query), chunk):
        q = query[s:s + chunk]
        dx, dy, dz = (q[:, None, k] - ref[None, :, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        j = d2.argmin(axis=1)                      # first minimiser = the smallest index
        idx[s:s + chunk] = j
        dist[s:s + chunk] = np.sqrt(d2[np.arange(len(q)), j])
    return dist, idx


def chamfer_ckdtree(gt, recon):
    """compute_chamfer's formula: (mean NN distance gt -> recon + mean NN distance recon -> gt) / 2 (cKDTree, fp64)"""
    from scipy.spatial import cKDTree

    d1, _ = cKDTree(recon).query(gt)
    d2, _ = cKDTree(gt).query(recon)
    return 0.5 * (float(d1.mean()) + float(d2.mean()))
