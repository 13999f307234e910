"""CPU model of the mesh components (the contract of dgnn_mesh_components / dgnn_mesh_component_measures / dgnn_mesh_component_keep,
include/dgnn_hip.h).

* connectivity: two faces are adjacent when they share an undirected edge, however many faces share it (a shared vertex alone does not
  connect); labels from scipy.sparse.csgraph.connected_components, renumbered in ascending order of each component's smallest face id;
* measures: the two per-face terms by the header's expressions in fp64 (numpy rounds every operation on its own), summed per component
  with math.fsum (the correctly rounded sum of the terms);
* the error bound of a device sum against that fsum, per component, derived below (not fitted);
* the keep rules; the mesh builders shared by the CPU and the GPU tests.
"""
from __future__ import annotations

import math

import numpy as np

from mesh_topology_model import tetra_faces

U = 2.0 ** -53   # unit roundoff of fp64


# ---- components --------------------------------------------------------------------------------------------------------------------
def _faces(faces):
    return np.asarray(faces, dtype=np.int64).reshape(-1, 3)


def face_adjacency(faces):
    """scipy CSR [F, F]: faces that hold the same undirected edge are chained in face order (enough for connectivity: every face of an
    edge reaches every other one)"""
    from scipy.sparse import coo_matrix

    f = _faces(faces)
    n = len(f)
    e = np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=1).reshape(-1, 2)
    lo, hi = e.min(axis=1), e.max(axis=1)
    owner = np.repeat(np.arange(n), 3)
    order = np.lexsort((owner, hi, lo))
    lo, hi, owner = lo[order], hi[order], owner[order]
    same = (lo[1:] == lo[:-1]) & (hi[1:] == hi[:-1])
    a, b = owner[:-1][same], owner[1:][same]
    return coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(n, n)).tocsr()


def renumber(labels):
    """any labelling -> the same partition numbered 0..K-1 in ascending order of each part's smallest index"""
    labels = np.asarray(labels)
    if len(labels) == 0:
        return np.zeros(0, dtype=np.int32), 0
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)].astype(np.int32), len(first)


def components(faces):
    """-> (comp int32 [F], K)"""
    from scipy.sparse.csgraph import connected_components

    f = _faces(faces)
    if len(f) == 0:
        return np.zeros(0, dtype=np.int32), 0
    _, lab = connected_components(face_adjacency(f), directed=False)
    return renumber(lab)


# ---- measures ----------------------------------------------------------------------------------------------------------------------
def face_terms(vertices, faces):
    """-> (area terms, volume terms) fp64 [F]: the expressions of include/dgnn_hip.h, operation by operation"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = _faces(faces)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    bx, by, bz = b[:, 0], b[:, 1], b[:, 2]
    cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
    ux, uy, uz = bx - ax, by - ay, bz - az
    wx, wy, wz = cx - ax, cy - ay, cz - az
    nx, ny, nz = uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    vol = ((ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx)) / 6.0
    return area, vol


def measures(vertices, faces, comp, k):
    """-> dict: n_faces int64 [K]; area, signed_volume fp64 [K] = math.fsum of the component's terms; area_bound, volume_bound fp64 [K].

    The bound on |device sum - fsum| for a component of n faces with terms t_i is (n + 3) * 2^-53 * sum |t_i|:
      n   the device adds the n terms with n - 1 fp64 additions (each piece and the total start from 0.0, and 0.0 + t is exact).  For ANY
          order of n - 1 additions the error is at most gamma_(n-1) * sum |t_i|, gamma_m = m u / (1 - m u), u = 2^-53 (Higham, Accuracy
          and Stability of Numerical Algorithms, §4.2), and gamma_(n-1) <= n u as long as n (n - 1) u <= 1, i.e. for n < 9e7 faces;
      1   fsum returns the exact sum rounded once: off by at most u |sum| <= u * sum |t_i|;
      2   the terms themselves: the device and numpy evaluate the same written expression with one rounding per operation (no fused
          multiply-add on either side), so sums, differences, products and the division by 6 agree bit for bit (IEEE 754).  The square
          root of the area term is the one operation whose rounding a device library may miss by one unit in the last place: 2 u |t_i|
          per term, 2 u * sum |t_i| in all.  (The volume term has no square root; it gets the same constant for one rule.)"""
    comp = np.asarray(comp, dtype=np.int64)
    ta, tv = face_terms(vertices, faces)
    out = dict(n_faces=np.bincount(comp, minlength=k).astype(np.int64), area=np.zeros(k), signed_volume=np.zeros(k), area_bound=np.zeros(k),
               volume_bound=np.zeros(k))
    order = np.argsort(comp, kind="stable")
    cuts = np.searchsorted(comp[order], np.arange(k + 1))
    for c in range(k):
        ids = order[cuts[c]:cuts[c + 1]]
        n = len(ids)
        out["area"][c] = math.fsum(ta[ids])
        out["signed_volume"][c] = math.fsum(tv[ids])
        out["area_bound"][c] = (n + 3) * U * math.fsum(np.abs(ta[ids]))
        out["volume_bound"][c] = (n + 3) * U * math.fsum(np.abs(tv[ids]))
    return out


# ---- the filter --------------------------------------------------------------------------------------------------------------------
def keep_mask(comp, counts, largest=False, min_faces=None):
    """bool [F]: `largest` = the component with the most faces, a tie to the smaller id; `min_faces` = components with at least that many"""
    comp, counts = np.asarray(comp, dtype=np.int64), np.asarray(counts, dtype=np.int64)
    assert bool(largest) != (min_faces is not None)
    if len(comp) == 0:
        return np.zeros(0, dtype=bool)
    if largest:
        return comp == int(np.argmax(counts))          # np.argmax: the first of equal maxima
    return counts[comp] >= int(min_faces)


def filter_faces(faces, comp, counts, **rule):
    keep = keep_mask(comp, counts, **rule)
    return _faces(faces)[keep].astype(np.int32), keep, int(keep.sum())


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def _mesh(faces, n_vertices, seed=0):
    v = np.random.default_rng(seed).random((n_vertices, 3)) * 4.0 - 1.0
    return v, np.asarray(faces, dtype=np.int32).reshape(-1, 3)


UNIT_TET = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def unit_tet(flip=False):
    """the unit tetrahedron's surface wound outward (signed volume +1/6), or with every face flipped (-1/6)"""
    f = np.array(tetra_faces((0, 1, 2, 3)), dtype=np.int32)       # (0, 1, 2, 3) is positively oriented
    return UNIT_TET.copy(), (f[:, ::-1].copy() if flip else f)


def strip(n_faces, seed=None):
    """a triangle strip of n_faces faces (face i = vertices i, i + 1, i + 2; one component), the face ORDER shuffled by a seeded
    permutation when `seed` is given: long parent chains, and the smallest face id is not at an end of the strip"""
    i = np.arange(n_faces)
    f = np.stack([i, i + 1, i + 2], axis=1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    if seed is not None:
        f = f[np.random.default_rng(seed).permutation(n_faces)]
    j = np.arange(n_faces + 2)
    x = (j // 2).astype(np.float64)
    v = np.stack([x, (j % 2) * 0.75, 0.01 * x * x], axis=1)
    return v, f.astype(np.int32)


def many_tets(n, seed=0):
    """n disjoint tetrahedron surfaces with interleaved face order: face j of tetrahedron t is face j * n + t"""
    rng = np.random.default_rng(seed)
    v = (rng.random((n, 1, 3)) * 50.0 + rng.random((n, 4, 3))).reshape(-1, 3)
    f = np.array([tetra_faces((4 * t, 4 * t + 1, 4 * t + 2, 4 * t + 3)) for t in range(n)], dtype=np.int32)   # [n, 4, 3]
    return v, np.ascontiguousarray(f.transpose(1, 0, 2)).reshape(-1, 3)


def crumbs_then_strip(n_crumbs=3, n_strip=700):
    """n_crumbs single faces first in face order, then a strip of n_strip faces: sorted by component the strip starts at position
    n_crumbs -- inside a chunk of 256 positions of the device's sums -- and runs over two chunk boundaries"""
    v, f = strip(n_strip)
    rng = np.random.default_rng(7)
    cv = rng.random((3 * n_crumbs, 3)) + 5.0
    cf = np.arange(3 * n_crumbs, dtype=np.int32).reshape(-1, 3)
    return np.concatenate([cv, v]), np.concatenate([cf, f + 3 * n_crumbs]).astype(np.int32)


def shells_and_crumbs():
    """two tetrahedron shells (vertices 0-3 and 10-13) with three single-face crumbs (vertices 4-9, 14-16) between their faces"""
    a, b = tetra_faces((0, 1, 2, 3)), tetra_faces((10, 11, 12, 13))
    faces = [a[0], (4, 5, 6), a[1], b[0], a[2], (7, 8, 9), b[1], b[2], a[3], (14, 15, 16), b[3]]
    return _mesh(faces, 17, seed=5)


def hand_made(case):
    """-> (vertices, faces, K)"""
    t = tetra_faces
    faces, k = {
        "empty": ([], 0),
        "one_face": ([(0, 1, 2)], 1),
        "shared_edge": ([(0, 1, 2), (2, 1, 3)], 1),
        "shared_vertex": ([(0, 1, 2), (2, 3, 4)], 2),
        "two_tets": (t((0, 1, 2, 3)) + t((4, 5, 6, 7)), 2),
        "glued_edge": (t((0, 1, 2, 3)) + t((0, 1, 6, 7)), 1),       # four faces meet on the edge (0, 1)
    }[case]
    v, f = _mesh(faces, 9, seed=len(case))
    return v, f, k


HAND_MADE = ["empty", "one_face", "shared_edge", "shared_vertex", "two_tets", "glued_edge"]
