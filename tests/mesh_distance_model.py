"""CPU model of the point-to-mesh distance and of the distance fold (the contract of dgnn_point_mesh_distance / dgnn_distance_fold /
dgnn_row_dot3, include/dgnn_hip.h).

* `distance`: the rule over ALL (point, face) pairs in numpy fp64, chunked over the points: no grid at all, so it states what the answer is
  whatever the binning.  Every product, sum, difference and division is one numpy operation, i.e. one fp64 rounding, in the header's order.
* `face_rule`: the same rule for one (point, face) pair over any number type: Python floats (fp64, one rounding per operation) and
  fractions.Fraction (no rounding at all), which is what the accuracy statement is measured against.
* `fold`: fixed_sum.h's order (serial sums over chunks of 256, then the chunk totals serially), inclusive thresholds.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

EDGES = ((0, 1), (1, 2), (2, 0))


# ---- one pair, any number type -----------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def segment_rule(p, u, v):
    """-> (d2, closest, 0 = inside the segment / 1 = at u / 2 = at v)"""
    e, w = _sub(v, u), _sub(p, u)
    ee, we = _dot(e, e), _dot(w, e)
    if we <= 0 or ee == 0:
        c, code = u, 1
    elif we >= ee:
        c, code = v, 2
    else:
        t = we / ee
        c, code = (u[0] + t * e[0], u[1] + t * e[1], u[2] + t * e[2]), 0
    d = _sub(p, c)
    return _dot(d, d), c, code


def face_rule(p, tri, ids=(0, 1, 2)):
    """p: 3 numbers, tri: 3 x 3 numbers, ids: the face's vertex ids -> (d2, closest, region)"""
    best = None
    for k, (i, j) in enumerate(EDGES):
        if ids[i] > ids[j]:
            i, j = j, i
        d2, c, code = segment_rule(p, tri[i], tri[j])
        if best is None or d2 < best[0]:
            best = (d2, c, 1 + k if code == 0 else 4 + (i if code == 1 else j))
    a = tri[0]
    n = _cross(_sub(tri[1], a), _sub(tri[2], a))
    nn = _dot(n, n)
    if nn > 0 and all(_dot(_cross(_sub(tri[j], tri[i]), _sub(p, tri[i])), n) > 0 for i, j in EDGES):
        s = _dot(_sub(p, a), n) / nn
        c = tuple(min(max(p[k] - s * n[k], min(t[k] for t in tri)), max(t[k] for t in tri)) for k in range(3))
        d = _sub(p, c)
        d2 = _dot(d, d)
        if d2 < best[0]:
            best = (d2, c, 0)
    return best


def distance_scalar(vertices, faces, p, number=float):
    """the lexicographic minimum of (d2, face) over all faces for ONE point, in `number` (float or Fraction) -> (d2, face, closest, region)"""
    v = [[number(float(x)) for x in row] for row in np.asarray(vertices, dtype=np.float64)]
    q = tuple(number(float(x)) for x in p)
    best = None
    for f, ids in enumerate(np.asarray(faces, dtype=np.int64)):
        d2, c, r = face_rule(q, [tuple(v[i]) for i in ids], tuple(int(i) for i in ids))
        if best is None or d2 < best[0]:
            best = (d2, f, c, r)
    return best


def sqrt_fraction(x):
    """sqrt of a non-negative Fraction as a float, to well below an ulp (integer square root of the scaled value)"""
    if x == 0:
        return 0.0
    k = 200
    return float(Fraction(math.isqrt((x.numerator << (2 * k)) // x.denominator), 1 << k))


# ---- all pairs, numpy ----------------------------------------------------------------------------------------------------------------
def _vdot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _vcross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _segment(p, u, v):
    e, w = v - u, p - u
    ee, we = _vdot(e, e), _vdot(w, e)
    at_u = (we <= 0) | (ee == 0)
    at_v = ~at_u & (we >= ee)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = we / ee
        c = u + t[..., None] * e
    c = np.where(at_u[..., None], u, np.where(at_v[..., None], v, c))
    d = p - c
    return _vdot(d, d), c, np.where(at_u, 1, np.where(at_v, 2, 0))


def _pairs(p, tri, ids):
    """p [n, 1, 3], tri [1, F, 3, 3], ids [1, F, 3] -> d2 [n, F], closest [n, F, 3], region [n, F]"""
    best = None
    for k, (i, j) in enumerate(EDGES):
        swap = ids[..., i] > ids[..., j]
        pu, pv = np.where(swap, j, i), np.where(swap, i, j)
        u = np.where(swap[..., None], tri[..., j, :], tri[..., i, :])
        v = np.where(swap[..., None], tri[..., i, :], tri[..., j, :])
        d2, c, code = _segment(p, u, v)
        reg = np.where(code == 0, 1 + k, 4 + np.where(code == 1, pu, pv))
        if best is None:
            best = [d2, c, reg]
        else:
            take = d2 < best[0]
            best = [np.where(take, d2, best[0]), np.where(take[..., None], c, best[1]), np.where(take, reg, best[2])]
    a = tri[..., 0, :]
    n = _vcross(tri[..., 1, :] - a, tri[..., 2, :] - a)
    nn = _vdot(n, n)
    ok = nn > 0
    for i, j in EDGES:
        ok = ok & (_vdot(_vcross(tri[..., j, :] - tri[..., i, :], p - tri[..., i, :]), n) > 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = _vdot(p - a, n) / nn
        c = np.minimum(np.maximum(p - s[..., None] * n, tri.min(axis=-2)), tri.max(axis=-2))
        d = p - c
        d2 = _vdot(d, d)
        take = ok & (d2 < best[0])
    return np.where(take, d2, best[0]), np.where(take[..., None], c, best[1]), np.where(take, 0, best[2])


def distance(vertices, faces, points, chunk=128):
    """-> (d2 fp64 [n], face int32 [n], closest fp64 [n, 3], region uint8 [n]) by all pairs; points of any float dtype are promoted exactly"""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    p = np.asarray(points).astype(np.float64).reshape(-1, 3)
    tri, ids = v[f][None], f[None]
    n = len(p)
    d2, face, closest, region = np.zeros(n), np.zeros(n, np.int32), np.zeros((n, 3)), np.zeros(n, np.uint8)
    for s in range(0, n, chunk):
        a, c, r = _pairs(p[s:s + chunk, None, :], tri, ids)
        k = np.argmin(a, axis=1)                       # the first minimum: ties to the lowest face
        rows = np.arange(len(k))
        d2[s:s + chunk], face[s:s + chunk], closest[s:s + chunk], region[s:s + chunk] = a[rows, k], k, c[rows, k], r[rows, k]
    return d2, face, closest, region


# ---- the fold ------------------------------------------------------------------------------------------------------------------------
def fixed_sum(x, chunk=256):
    x = np.asarray(x, dtype=np.float64)
    total = 0.0
    for s in range(0, len(x), chunk):
        part = 0.0
        for y in x[s:s + chunk]:
            part += float(y)
        total += part
    return total


def fold(dist, cosine=None, thresholds=()):
    """-> (sum of dist, sum of |cosine| (0.0 without), max of dist (0.0 for none), [#{dist <= t} for t in thresholds])"""
    d = np.asarray(dist, dtype=np.float64)
    return (fixed_sum(d), fixed_sum(np.abs(np.asarray(cosine, dtype=np.float64))) if cosine is not None else 0.0,
            float(d.max()) if len(d) else 0.0, [int((d <= t).sum()) for t in thresholds])


def row_dot3(a, ia, b, ib):
    x, y = np.asarray(a, dtype=np.float64)[np.asarray(ia, dtype=np.int64)], np.asarray(b, dtype=np.float64)[np.asarray(ib, dtype=np.int64)]
    return _vdot(x, y)


def key(name, t):
    return "%s@%g" % (name, t)


def metrics_from_folds(fold_ab, n_a, fold_ba, n_b, thresholds, with_normals=True):
    """the keys of ops.surface_metrics from the two folds (A -> B over n_a samples, B -> A over n_b)"""
    sa, ca, ma, ka = fold_ab
    sb, cb, mb, kb = fold_ba
    out = {"accuracy": sa / n_a, "completeness": sb / n_b}
    out["chamfer_mesh"] = 0.5 * (out["accuracy"] + out["completeness"])
    out["hausdorff"] = max(ma, mb)
    for t, x, y in zip(thresholds, ka, kb):
        p, r = x / n_a, y / n_b
        out[key("precision", t)], out[key("recall", t)] = p, r
        out[key("fscore", t)] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    if with_normals:
        out["normal_consistency"] = 0.5 * (ca / n_a + cb / n_b)
    return out


# ---- meshes and points of the tests ----------------------------------------------------------------------------------------------------
def degenerate_mesh():
    """a cube with, appended: a collinear face, a face with two equal ids, a face of one id, a duplicate of face 0 and a far needle"""
    from mesh_contains_model import cube

    v, f = cube(0.0, 4.0)
    v = np.concatenate([v, [[5.0, 5.0, 5.0], [6.0, 6.0, 6.0], [7.0, 7.0, 7.0], [5.0, 1.0, 1.0]]])
    extra = [[8, 9, 10], [8, 11, 8], [11, 11, 11], list(f[0]), [9, 8, 8]]
    return v, np.concatenate([f, np.array(extra, dtype=np.int32)])


def flat_mesh(n=12, seed=0):
    """a fan of triangles in the plane z = 0.25"""
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2))
    v = np.concatenate([xy, np.full((n, 1), 0.25)], axis=1)
    f = np.array([[0, i, i + 1] for i in range(1, n - 1)], dtype=np.int32)
    return v, f


def unequal_mesh(n_small=500, seed=0):
    """one triangle spanning the box among n_small small ones"""
    rng = np.random.default_rng(seed)
    c = rng.random((n_small, 1, 3))
    small = c + 0.02 * (rng.random((n_small, 3, 3)) - 0.5)
    v = np.concatenate([[[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.5, 0.5, 1.0]], small.reshape(-1, 3)])
    f = np.arange(3 * (n_small + 1), dtype=np.int32).reshape(-1, 3)
    return v, f


def query_points(vertices, faces, n_uniform, seed):
    """uniform in three times the box (most outside it); far outside, 100 extents away, on one axis and on all; points exactly on faces,
    edges and vertices; the centre; the referenced vertices themselves -> fp64 [n, 3]"""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    used = v[np.unique(f)]
    lo, hi = used.min(axis=0), used.max(axis=0)
    ext = np.where(hi > lo, hi - lo, (hi - lo).max() if (hi - lo).max() > 0 else 1.0)
    mid = 0.5 * (lo + hi)
    rng = np.random.default_rng(seed)
    parts = [mid + 3.0 * ext * (rng.random((n_uniform, 3)) - 0.5)]
    far = []
    for a in range(3):
        for sgn in (-1.0, 1.0):
            q = mid + 0.3 * ext * (rng.random(3) - 0.5)
            q[a] = mid[a] + sgn * 100.0 * ext[a]
            far.append(q)
    far += [mid + 100.0 * ext, mid - 100.0 * ext, mid + 100.0 * ext * np.array([1.0, -1.0, 1.0])]
    parts.append(np.array(far))
    tri = v[f[:: max(1, len(f) // 150)]]
    w = rng.dirichlet((1, 1, 1), size=len(tri))
    parts.append((w[:, :, None] * tri).sum(axis=1))                                  # on faces
    parts += [0.5 * (tri[:, a] + tri[:, b]) for a, b in EDGES]                       # on edges
    parts += [0.25 * tri[:, 0] + 0.75 * tri[:, 1], mid[None], used[:400]]
    return np.concatenate(parts, axis=0)


# ---- the device's search, restated: the same cells, shells, skip rule and stopping bound (slow: for small cases) -------------------------
MARGIN, SHRINK = 2.0 ** -46, 1.0 - 2.0 ** -50


def grid_frame(vertices, faces, R):
    v = np.asarray(vertices, dtype=np.float64)
    used = v[np.unique(np.asarray(faces, dtype=np.int64))]
    lo, hi = used.min(axis=0), used.max(axis=0)
    ext = hi - lo
    longest = ext.max()
    n, h, inv = np.ones(3, np.int64), np.zeros(3), np.zeros(3)
    for a in range(3):
        cells = math.ceil(ext[a] / (longest / R)) if longest > 0 else 1.0
        cells = min(max(cells, 1), R)
        n[a], h[a], inv[a] = cells, ext[a] / cells, (cells / ext[a] if ext[a] > 0 else 0.0)
    return dict(lo=lo, hi=hi, n=n, h=h, inv=inv, mag=max(np.abs(lo).max(), np.abs(hi).max()))


def grid_cell(g, a, x):
    f = (x - g["lo"][a]) * g["inv"][a]
    return 0 if not f > 0 else (int(g["n"][a]) - 1 if f >= g["n"][a] else int(f))


def distance_grid(vertices, faces, points, R):
    """-> (d2, face, closest, region, stats) as the device's search computes them; stats = (max shells, shells, evaluations)"""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    g = grid_frame(v, f, R)
    tri = v[f]
    blo = np.array([[grid_cell(g, a, tri[t, :, a].min()) for a in range(3)] for t in range(len(f))])
    bhi = np.array([[grid_cell(g, a, tri[t, :, a].max()) for a in range(3)] for t in range(len(f))])
    cells = {}
    for t in range(len(f)):
        for x in range(blo[t, 0], bhi[t, 0] + 1):
            for y in range(blo[t, 1], bhi[t, 1] + 1):
                for z in range(blo[t, 2], bhi[t, 2] + 1):
                    cells.setdefault((x, y, z), []).append(t)
    vl = [[float(x) for x in row] for row in v]
    out, shell_max, shell_sum, evals = [], 0, 0, 0
    n = [int(x) for x in g["n"]]
    for p in np.asarray(points, dtype=np.float64).reshape(-1, 3):
        q = tuple(float(x) for x in p)
        c = [grid_cell(g, a, q[a]) for a in range(3)]
        eps = MARGIN * max(g["mag"], max(abs(x) for x in q))
        out2 = [max(max(g["lo"][a] - q[a], q[a] - g["hi"][a]) - eps, 0.0) ** 2 for a in range(3)]
        best, s = None, 0
        while s < max(n):
            lo_ = [max(c[a] - s, 0) for a in range(3)]
            hi_ = [min(c[a] + s, n[a] - 1) for a in range(3)]
            for x in range(lo_[0], hi_[0] + 1):
                for y in range(lo_[1], hi_[1] + 1):
                    # the cells at Chebyshev distance exactly s: the whole column when x or y is at distance s, else the column's two ends
                    on_shell = abs(x - c[0]) == s or abs(y - c[1]) == s
                    for z in (range(lo_[2], hi_[2] + 1) if on_shell else [z for z in (c[2] - s, c[2] + s) if lo_[2] <= z <= hi_[2]]):
                        for t in cells.get((x, y, z), ()):
                            if s > 0 and all(max(blo[t, a], c[a] - s + 1) <= min(bhi[t, a], c[a] + s - 1) for a in range(3)):
                                continue
                            ids = tuple(int(i) for i in f[t])
                            d2, cl, r = face_rule(q, [tuple(vl[i]) for i in ids], ids)
                            evals += 1
                            if best is None or d2 < best[0] or (d2 == best[0] and t < best[1]):
                                best = (d2, t, cl, r)
            b2, open_side = math.inf, False
            for a in range(3):
                rest = out2[0 if a else 1] + out2[1 if a == 2 else 2]
                if lo_[a] > 0:
                    open_side = True
                    b = max((q[a] - (g["lo"][a] + float(lo_[a]) * g["h"][a])) - eps, 0.0)
                    b2 = min(b2, b * b + rest)
                if hi_[a] < n[a] - 1:
                    open_side = True
                    b = max(((g["lo"][a] + float(hi_[a] + 1) * g["h"][a]) - q[a]) - eps, 0.0)
                    b2 = min(b2, b * b + rest)
            s += 1
            if not open_side or (best is not None and best[0] < b2 * SHRINK):
                break
        shell_max, shell_sum = max(shell_max, s), shell_sum + s
        out.append(best)
    return (np.array([b[0] for b in out]), np.array([b[1] for b in out], np.int32), np.array([b[2] for b in out], dtype=np.float64).reshape(-1, 3),
            np.array([b[3] for b in out], np.uint8), (shell_max, shell_sum, evals))


def uv_sphere(n_lat, n_lon):
    """a closed unit sphere of 2 n_lon (n_lat - 1) faces"""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon))], -1).reshape(-1, 3)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]])
    idx = 1 + np.arange((n_lat - 1) * n_lon).reshape(n_lat - 1, n_lon)
    nxt = np.roll(idx, -1, axis=1)
    quads = np.stack([idx[:-1], idx[1:], nxt[1:], idx[:-1], nxt[1:], nxt[:-1]], -1).reshape(-1, 3)
    top = np.stack([np.zeros(n_lon, np.int64), idx[0], nxt[0]], -1)
    bot = np.stack([np.full(n_lon, len(v) - 1), nxt[-1], idx[-1]], -1)
    return v, np.concatenate([top, quads, bot]).astype(np.int32)


def deep_queries(seed=0):
    """queries about the unit sphere, in groups: "near" (40, on the sphere scaled by 1.01), "inside" (40, uniform in the box of edge 2.2, with
    the centre first), "outside" (12: 100 extents away, on one axis and on all axes), "around" (12: about 3 extents away)"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(40, 3))
    near = 1.01 * d / np.linalg.norm(d, axis=1, keepdims=True)
    inside = 2.2 * (rng.random((40, 3)) - 0.5)
    inside[0] = 0.0
    out = []
    for a in range(3):
        for sgn in (-1.0, 1.0):
            q = 0.6 * (rng.random(3) - 0.5)
            q[a] = sgn * 200.0
            out.append(q)
    out += [200.0 * np.array(sg) for sg in ((1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1), (1, 1, -1), (-1, -1, -1))]
    around = 6.0 * (rng.random((12, 3)) - 0.5) + 6.0 * np.sign(rng.random((12, 3)) - 0.5)
    return {"near": near, "inside": inside, "outside": np.array(out), "around": around}
