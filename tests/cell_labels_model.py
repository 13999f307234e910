"""CPU model of the ground-truth cell labels (the contract of dgnn_tet_sample_points / dgnn_cell_labels, include/dgnn_hip.h):
the numpy restatement of the sampler, one fp64 rounding per operation in the order the header writes them, composed with the all-pairs
occupancy model mesh_contains_model.contains.
"""
from __future__ import annotations

import numpy as np

import mesh_contains_model as mc
from mesh_metrics_model import mm_hash


def barycentrics(seed, first_counter, n):
    """the folded (s, t, u) of n consecutive samples, the first with counter `first_counter` (a Python int, taken mod 2^64) -> fp64 [n, 3]"""
    with np.errstate(over="ignore"):
        c = np.uint64(first_counter % 2 ** 64) + np.uint64(3) * np.arange(n, dtype=np.uint64)
        s = mc._u01(mm_hash(seed, c))
        t = mc._u01(mm_hash(seed, c + np.uint64(1)))
        u = mc._u01(mm_hash(seed, c + np.uint64(2)))
    flip = s + t > 1
    s, t = np.where(flip, 1 - s, s), np.where(flip, 1 - t, t)
    st = s + t
    a = t + u > 1
    b = ~a & (st + u > 1)
    s2 = np.where(b, (1 - t) - u, s)
    t2 = np.where(a, 1 - u, t)
    u2 = np.where(a, (1 - s) - t, np.where(b, (st + u) - 1, u))
    return np.stack([s2, t2, u2], axis=1)


def sample_points(vertices, tetrahedra, k, seed, tet_offset=0):
    """-> fp64 [T k, 3]: row t k + j = sample j of tet t, counter 3 ((tet_offset + t) k + j) + 1"""
    v = np.asarray(vertices, dtype=np.float64)
    tets = np.asarray(tetrahedra, dtype=np.int64).reshape(-1, 4)
    out = np.zeros((len(tets), k, 3))
    for i, tet in enumerate(tets):
        b = barycentrics(seed, 3 * ((int(tet_offset) + i) * k) + 1, k)
        p0 = v[tet[0]]
        e1, e2, e3 = v[tet[1]] - p0, v[tet[2]] - p0, v[tet[3]] - p0
        out[i] = ((b[:, 0:1] * e1 + b[:, 1:2] * e2) + b[:, 2:3] * e3) + p0
    return out.reshape(-1, 3)


def labels(mesh_vertices, mesh_faces, vertices, tetrahedra, k, seed, tet_offset=0, R=512):
    """-> (count int32 [T], inside_perc, outside_perc fp64 [T], n_disagree)"""
    n_tets = len(np.asarray(tetrahedra).reshape(-1, 4))
    pts = sample_points(vertices, tetrahedra, k, seed, tet_offset)
    inside, n_disagree = mc.contains(mesh_vertices, mesh_faces, pts, R) if n_tets else (np.zeros(0, dtype=bool), 0)
    count = inside.reshape(n_tets, k).sum(axis=1).astype(np.int32)
    return count, count.astype(np.float64) / float(k), (k - count).astype(np.float64) / float(k), n_disagree
