"""CPU model of the mesh occupancy query and of the evaluation-sample generators (the contract of dgnn_mesh_contains / dgnn_box_points /
dgnn_jitter_points / dgnn_face_normals, include/dgnn_hip.h).

* contains: ALL PAIRS of (point, triangle) in fp64, chunked over the points: no grid at all, so it states what the answer is whatever
  the binning; `candidates` + `contains_from_candidates` evaluate the same expressions over the lists of a host-side grid, to show that
  the binning does not matter;
* generators: the hash is mesh_metrics_model.mm_hash.
"""
from __future__ import annotations

import numpy as np

from mesh_metrics_model import mm_hash


# ---- the frame -------------------------------------------------------------------------------------------------------------------
def frame(vertices, faces, R=512):
    """-> (scale [3], translate [3]) over the vertices the faces reference"""
    tri = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)].reshape(-1, 3)
    lo, hi = tri.min(axis=0), tri.max(axis=0)
    scale = (R - 1) / (hi - lo)
    m = scale * lo
    return scale, 0.5 - m


def rescale(a, scale, translate):
    m = scale * np.asarray(a, dtype=np.float64)
    return m + translate


# ---- per (point, triangle) pair ----------------------------------------------------------------------------------------------------
def _pair_counts(p, t):
    """p [..., 3] rescaled points, t [..., 3, 3] rescaled triangles, broadcastable -> (above, below) bool arrays"""
    t1, t2, t3 = t[..., 0, :], t[..., 1, :], t[..., 2, :]
    with np.errstate(invalid="ignore", over="ignore"):
        a00, a01 = t1[..., 0] - t3[..., 0], t2[..., 0] - t3[..., 0]
        a10, a11 = t1[..., 1] - t3[..., 1], t2[..., 1] - t3[..., 1]
        y0, y1 = p[..., 0] - t3[..., 0], p[..., 1] - t3[..., 1]
        det = a00 * a11 - a01 * a10
        sd, ad = np.sign(det), np.abs(det)
        u = (a11 * y0 - a01 * y1) * sd
        v = (-a10 * y0 + a00 * y1) * sd
        uv = u + v
        hit = (ad != 0) & (0 < u) & (u < ad) & (0 < v) & (v < ad) & (0 < uv) & (uv < ad)
        v1, v2 = t3 - t1, t2 - t1
        n0 = v1[..., 1] * v2[..., 2] - v1[..., 2] * v2[..., 1]
        n1 = v1[..., 2] * v2[..., 0] - v1[..., 0] * v2[..., 2]
        n2 = v1[..., 0] * v2[..., 1] - v1[..., 1] * v2[..., 0]
        alpha = n0 * (t1[..., 0] - p[..., 0]) + n1 * (t1[..., 1] - p[..., 1])
        an, sn = np.abs(n2), np.sign(n2)
        depth = np.where(an != 0, t1[..., 2] * an + alpha * sn, np.nan)
        rhs = p[..., 2] * an
        return hit & (depth >= rhs), hit & (depth < rhs)


def _finish(n_above, n_below, inside_box):
    c1, c2 = (n_above % 2 == 1) & inside_box, (n_below % 2 == 1) & inside_box
    return c1 & c2, int((c1 != c2).sum())


def _inside_box(p, R):
    with np.errstate(invalid="ignore"):
        return ((0 <= p) & (p <= R)).all(axis=1)


def contains(vertices, faces, points, R=512, chunk=256):
    """-> (contains bool [n], n_disagree) by all pairs; points of any float dtype are promoted exactly"""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    scale, translate = frame(v, f, R)
    tri = rescale(v, scale, translate)[f]
    p = rescale(np.asarray(points).astype(np.float64), scale, translate)
    na, nb = np.zeros(len(p), dtype=np.int64), np.zeros(len(p), dtype=np.int64)
    for s in range(0, len(p), chunk):
        above, below = _pair_counts(p[s:s + chunk, None, :], tri[None])
        na[s:s + chunk], nb[s:s + chunk] = above.sum(axis=1), below.sum(axis=1)
    return _finish(na, nb, _inside_box(p, R))


# ---- the same through a grid's candidate lists ---------------------------------------------------------------------------------------
def candidates(vertices, faces, points, R=512, shift=0):
    """(point index, triangle index) pairs a grid on int(coord) >> shift offers: a triangle is in every cell its xy box touches (cells
    clamped to [0, R - 1]), a point inside the box with int(x), int(y) < R reads its own cell"""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    scale, translate = frame(v, f, R)
    tri = rescale(v, scale, translate)[f]
    p = rescale(np.asarray(points).astype(np.float64), scale, translate)
    lo = np.clip(tri[:, :, :2].min(axis=1).astype(np.int64), 0, R - 1) >> shift
    hi = np.clip(tri[:, :, :2].max(axis=1).astype(np.int64), 0, R - 1) >> shift
    ok = _inside_box(p, R)
    with np.errstate(invalid="ignore"):
        ok &= (p[:, 0] < R) & (p[:, 1] < R)
    idx = np.nonzero(ok)[0]
    c = p[idx, :2].astype(np.int64) >> shift
    pi, ti = [], []
    for s in range(0, len(idx), 256):
        cc = c[s:s + 256, None, :]
        m = ((lo[None] <= cc) & (cc <= hi[None])).all(axis=2)
        a, b = np.nonzero(m)
        pi.append(idx[s + a])
        ti.append(b)
    return (np.concatenate(pi), np.concatenate(ti)) if pi else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def contains_from_candidates(vertices, faces, points, pairs, R=512):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    scale, translate = frame(v, f, R)
    tri = rescale(v, scale, translate)[f]
    p = rescale(np.asarray(points).astype(np.float64), scale, translate)
    pi, ti = pairs
    above, below = _pair_counts(p[pi], tri[ti])
    na = np.bincount(pi[above], minlength=len(p))
    nb = np.bincount(pi[below], minlength=len(p))
    return _finish(na, nb, _inside_box(p, R))


# ---- generators ----------------------------------------------------------------------------------------------------------------------
def _u01(h):
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _u01_open0(h):
    return ((h >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def box_points(n, boxsize, seed):
    j = np.arange(3 * n, dtype=np.uint64)
    return (boxsize * (_u01(mm_hash(seed, j + np.uint64(1))) - 0.5)).reshape(n, 3)


def jitter_points(points64, sigma, seed):
    p = np.asarray(points64, dtype=np.float64)
    j = np.arange(p.size, dtype=np.uint64)
    u1 = _u01_open0(mm_hash(seed, np.uint64(2) * j + np.uint64(1)))
    u2 = _u01(mm_hash(seed, np.uint64(2) * j + np.uint64(2)))
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
    return p + (sigma * z).reshape(p.shape)


def face_normals(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    ln = np.sqrt((n * n).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((ln > 0)[:, None], n / ln[:, None], 0.0)


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    v = np.array([[0.1, 0.2, 0.05], [1.3, 0.15, 0.2], [0.4, 1.1, 0.1], [0.55, 0.45, 1.2]])
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int32)


def cube(lo=0.0, hi=4.0):
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], dtype=np.float64)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                 dtype=np.int32)
    return v, f


def lattice(lo, hi):
    """the integer points [lo, hi)^3 -> fp64 [n, 3]"""
    return np.stack(np.meshgrid(*[np.arange(lo, hi, dtype=np.float64)] * 3, indexing="ij"), -1).reshape(-1, 3)


def sphere_interface(n_points=300, seed=0):
    """the closed interface of mesh_metrics_model.random_scene(n_points) labelled by the sphere, on its own compacted vertices"""
    import mesh_metrics_model as mm

    sc = mm.random_scene(n_points, seed)
    ids = mm.interface_ids(mm.sphere_labels(sc), sc["nfacets"])
    tri = sc["facets"][ids].astype(np.int64)
    kept, inv = np.unique(tri, return_inverse=True)
    return sc["vertices"][kept], inv.reshape(-1, 3).astype(np.int32)


def adversarial_points(vertices, faces, n_uniform, seed, pad=0.1):
    """uniform points in the padded box; every vertex, edge midpoint and face centroid; the eight box corners; points just outside each
    side; NaN and +-inf rows -> fp64 [n, 3]"""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    used = v[np.unique(f)]
    lo, hi = used.min(axis=0), used.max(axis=0)
    ext = hi - lo
    rng = np.random.default_rng(seed)
    parts = [lo - pad * ext + rng.random((n_uniform, 3)) * (1 + 2 * pad) * ext, used]
    tri = v[f]
    parts += [0.5 * (tri[:, a] + tri[:, b]) for a, b in ((0, 1), (1, 2), (2, 0))]
    parts.append(tri.mean(axis=1))
    parts.append(np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]))
    mid = 0.5 * (lo + hi)
    out = []
    for a in range(3):
        for side, sgn in ((lo, -1.0), (hi, 1.0)):
            for eps in (1e-12, 1e-6, 1e-3):
                q = mid.copy()
                q[a] = side[a] + sgn * eps * ext[a]
                out.append(q)
            q = mid.copy()
            q[a] = np.nextafter(side[a], side[a] + sgn)
            out.append(q)
    parts.append(np.array(out))
    odd = np.tile(mid, (9, 1))
    for a in range(3):
        odd[3 * a, a], odd[3 * a + 1, a], odd[3 * a + 2, a] = np.nan, np.inf, -np.inf
    parts.append(odd)
    return np.concatenate(parts, axis=0)
