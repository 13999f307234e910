"""The k-nearest-neighbour rule and the scan operations on it (include/dgnn_hip.h) restated in numpy, operation for operation:
`knn` over all pairs, `knn_grid` the device's shell search with its counts, `mean_distance`, `outlier_mask` in fixed_sum.h's order, `normals`
by fixed-sweep Jacobi, and the point clouds of the tests.  No GPU, no torch."""
import functools
import math

import numpy as np

MAX_K = 64
MARGIN, SHRINK = 2.0 ** -46, 1.0 - 2.0 ** -50
FIXED_SUM_CHUNK = 256
JACOBI_SWEEPS = 6


def default_resolution(n_points):
    return max(1, min(512, int(round(0.175 * float(n_points) ** 0.5))))


# ---- the rule over all pairs --------------------------------------------------------------------------------------------------------
def d2_matrix(queries, points):
    q, p = np.asarray(queries, dtype=np.float64).reshape(-1, 3), np.asarray(points, dtype=np.float64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        dx, dy, dz = (q[:, None, a] - p[None, :, a] for a in range(3))
        return (dx * dx + dy * dy) + dz * dz


def full_order(points, queries=None):
    """every query's candidates in ascending (d2, index): (index int64 [Q, m], d2 [Q, m]); m = n, or n - 1 with the points as their own queries
    (query i leaves out point i by index)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    d2 = d2_matrix(p if queries is None else queries, p)
    order = np.argsort(d2, axis=1, kind="stable")          # ties keep the ascending index
    if queries is None and len(p):
        order = order[order != np.arange(len(p))[:, None]].reshape(len(p), len(p) - 1)
    return order, np.take_along_axis(d2, order, axis=1)


def _first_k(order, d2s, k):
    q, m = order.shape
    idx, d2 = np.full((q, k), -1, np.int32), np.full((q, k), np.inf)
    idx[:, :min(k, m)], d2[:, :min(k, m)] = order[:, :k], d2s[:, :k]
    return idx, d2


def knn(points, k, queries=None, ordered=None):
    """-> (idx int32 [Q, k], d2 fp64 [Q, k]); ordered: full_order's result, when the caller keeps it"""
    if not 1 <= k <= MAX_K:
        raise ValueError("k = %d outside [1, %d]" % (k, MAX_K))
    order, d2s = full_order(points, queries) if ordered is None else ordered
    return _first_k(order, d2s, k)


# ---- the device's search, restated: the same cells, shells and stopping bound ----------------------------------------------------------
def grid_frame(points, R):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = hi - lo
    longest = ext.max()
    n, h, inv = np.ones(3, np.int64), np.zeros(3), np.zeros(3)
    for a in range(3):
        cells = math.ceil(ext[a] / (longest / R)) if longest > 0 else 1.0
        cells = min(max(cells, 1), R)
        with np.errstate(over="ignore"):
            n[a], h[a], inv[a] = cells, ext[a] / cells, (cells / ext[a] if ext[a] > 0 else 0.0)
        if not (np.isfinite(inv[a]) and np.isfinite(ext[a])):
            n[a], h[a], inv[a] = 1, ext[a], 0.0
    return dict(lo=lo, hi=hi, n=n, h=h, inv=inv, mag=max(np.abs(lo).max(), np.abs(hi).max()))


def grid_cells(g, x):
    """the cell of every row of x [m, 3]"""
    f = (np.asarray(x, dtype=np.float64).reshape(-1, 3) - g["lo"]) * g["inv"]
    top = (g["n"] - 1).astype(np.float64)
    return np.where(~(f > 0), 0.0, np.where(f >= g["n"], top, np.trunc(np.minimum(f, top)))).astype(np.int64)


def knn_grid(points, k, R, queries=None, ordered=None):
    """-> (idx, d2, (shells, candidates)) as the device's search at resolution R > 0 computes them: shells read and records of the cells read
    (the query's own included), summed over the queries"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    order, d2s = full_order(p, queries) if ordered is None else ordered
    q_all = p if queries is None else np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    g = grid_frame(p, R)
    n = [int(x) for x in g["n"]]
    pc, qc = grid_cells(g, p), grid_cells(g, q_all)
    lo, hi, h = ([float(x) for x in g[key]] for key in ("lo", "hi", "h"))
    idx, d2 = np.full((len(q_all), k), -1, np.int32), np.full((len(q_all), k), np.inf)
    shells = cands = 0
    for i in range(len(q_all)):
        q = [float(x) for x in q_all[i]]
        c = [int(x) for x in qc[i]]
        cheb = np.abs(pc - qc[i]).max(axis=1)
        per_shell = np.bincount(cheb, minlength=max(n))
        cheb_sorted = cheb[order[i]]
        eps = MARGIN * max(g["mag"], max(abs(x) for x in q))
        out2 = [max(max(lo[a] - q[a], q[a] - hi[a]) - eps, 0.0) ** 2 for a in range(3)]
        s = 0
        while s < max(n):
            cands += int(per_shell[s])
            got = np.flatnonzero(cheb_sorted <= s)[:k]
            lo_ = [max(c[a] - s, 0) for a in range(3)]
            hi_ = [min(c[a] + s, n[a] - 1) for a in range(3)]
            b2, open_side = math.inf, False
            for a in range(3):
                rest = out2[0 if a else 1] + out2[1 if a == 2 else 2]
                if lo_[a] > 0:
                    open_side = True
                    b = max((q[a] - (lo[a] + float(lo_[a]) * h[a])) - eps, 0.0)
                    b2 = min(b2, b * b + rest)
                if hi_[a] < n[a] - 1:
                    open_side = True
                    b = max(((lo[a] + float(hi_[a] + 1) * h[a]) - q[a]) - eps, 0.0)
                    b2 = min(b2, b * b + rest)
            s += 1
            if not open_side or (len(got) == k and float(d2s[i, got[-1]]) < b2 * SHRINK):
                break
        shells += s
        idx[i, :len(got)], d2[i, :len(got)] = order[i, got], d2s[i, got]
    return idx, d2, (shells, cands)


# ---- on the lists ----------------------------------------------------------------------------------------------------------------------
def mean_distance(d2, idx):
    d2, idx = np.asarray(d2, dtype=np.float64), np.asarray(idx)
    s, cnt = np.zeros(len(d2)), np.zeros(len(d2))
    for r in range(d2.shape[1]):
        ok = idx[:, r] >= 0
        s = np.where(ok, s + np.sqrt(np.where(ok, d2[:, r], 0.0)), s)
        cnt = cnt + ok
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / cnt


def fixed_sum(x):
    """fixed_sum.h: serial sums over chunks of 256, then the chunk totals serially"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    part = [np.cumsum(x[t:t + FIXED_SUM_CHUNK])[-1] for t in range(0, len(x), FIXED_SUM_CHUNK)]
    return float(np.cumsum(part)[-1]) if part else 0.0


def outlier_mask(points, k=16, std_ratio=2.0, ordered=None):
    """-> (keep bool [n], dict of mean_distance, mu, sigma, threshold, n_removed)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    if n < 2:
        raise ValueError("at least 2 points are needed")
    idx, d2 = knn(p, min(k, n - 1), ordered=ordered)
    m = mean_distance(d2, idx)
    mu = fixed_sum(m) / float(n)
    dev = m - mu
    sigma = math.sqrt(fixed_sum(dev * dev) / float(n))
    threshold = mu + float(std_ratio) * sigma
    keep = m <= threshold
    return keep, dict(mean_distance=m, mu=mu, sigma=sigma, threshold=threshold, n_removed=int(n - keep.sum()))


def _serial_sum(x):
    """over axis 1, in order"""
    return np.cumsum(x, axis=1)[:, -1]


def _rotate(app, aqq, apq, arp, arq, vp, vq):
    """one Jacobi rotation of every matrix of a batch, skipped where a_pq == 0; vp, vq [N, 3]: the columns p and q of V"""
    skip = apq == 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        new = (app - t * apq, aqq + t * apq, np.zeros_like(apq), c * arp - s * arq, s * arp + c * arq,
               c[:, None] * vp - s[:, None] * vq, s[:, None] * vp + c[:, None] * vq)
    old = (app, aqq, apq, arp, arq, vp, vq)
    return tuple(np.where(skip[:, None] if o.ndim == 2 else skip, o, w) for o, w in zip(old, new))


def pca(nbhd, sweeps=JACOBI_SWEEPS):
    """nbhd [N, m, 3], each neighbourhood in its order -> (normal [N, 3] with its component of largest magnitude positive, eigenvalues [N, 3]
    ascending): the centroid, the six sums, `sweeps` cyclic Jacobi sweeps, the column of the smallest diagonal entry"""
    P = np.asarray(nbhd, dtype=np.float64)
    c = _serial_sum(P) / float(P.shape[1])
    d = P - c[:, None, :]
    dx, dy, dz = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    a00, a11, a22, a01, a02, a12 = (_serial_sum(x) for x in (dx * dx, dy * dy, dz * dz, dx * dy, dx * dz, dy * dz))
    N = len(P)
    v = [np.tile(np.eye(3)[:, j], (N, 1)) for j in range(3)]          # the columns of V
    for _ in range(sweeps):
        a00, a11, a01, a02, a12, v[0], v[1] = _rotate(a00, a11, a01, a02, a12, v[0], v[1])
        a00, a22, a02, a01, a12, v[0], v[2] = _rotate(a00, a22, a02, a01, a12, v[0], v[2])
        a11, a22, a12, a01, a02, v[1], v[2] = _rotate(a11, a22, a12, a01, a02, v[1], v[2])
    diag = np.stack([a00, a11, a22], axis=1)
    col = np.zeros(N, np.int64)
    col = np.where(diag[:, 1] < diag[np.arange(N), col], 1, col)
    col = np.where(diag[:, 2] < diag[np.arange(N), col], 2, col)
    e0, e1, e2 = a00, a11, a22          # ascending, ties by column: three strict exchanges
    e0, e1 = np.where(e1 < e0, e1, e0), np.where(e1 < e0, e0, e1)
    e1, e2 = np.where(e2 < e1, e2, e1), np.where(e2 < e1, e1, e2)
    e0, e1 = np.where(e1 < e0, e1, e0), np.where(e1 < e0, e0, e1)
    nrm = np.stack(v, axis=2)[np.arange(N), :, col]
    length = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
    nrm = nrm / length[:, None]
    mag = np.abs(nrm)
    big = np.zeros(N, np.int64)
    big = np.where(mag[:, 1] > mag[np.arange(N), big], 1, big)
    big = np.where(mag[:, 2] > mag[np.arange(N), big], 2, big)
    nrm = np.where((nrm[np.arange(N), big] < 0.0)[:, None], -nrm, nrm)
    return nrm, np.stack([e0, e1, e2], axis=1)


def normals(points, k=16, sensors=None, ordered=None, sweeps=JACOBI_SWEEPS):
    """-> (normals [n, 3], eigenvalues [n, 3]): pca of (the point, then its min(k, n - 1) neighbours in rank order), turned towards the sensor"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    if n < 3:
        raise ValueError("at least 3 points are needed")
    idx, _ = knn(p, min(k, n - 1), ordered=ordered)
    assert (idx >= 0).all()
    nrm, eig = pca(np.concatenate([p[:, None, :], p[idx]], axis=1), sweeps)
    if sensors is not None:
        t = np.asarray(sensors, dtype=np.float64).reshape(-1, 3) - p
        dot = (nrm[:, 0] * t[:, 0] + nrm[:, 1] * t[:, 1]) + nrm[:, 2] * t[:, 2]
        nrm = np.where((dot < 0.0)[:, None], -nrm, nrm)
    return nrm, eig


# ---- the point clouds --------------------------------------------------------------------------------------------------------------
def fibonacci_sphere(n):
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    r, phi = np.sqrt(1.0 - z * z), i * (np.pi * (3.0 - 5.0 ** 0.5))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def _uniform():
    return np.random.default_rng(1).random((1200, 3))


def _lattice():
    return np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)


def _duplicates():
    rng = np.random.default_rng(2)
    p = rng.random((240, 3))
    p[rng.permutation(240)[:40]] = p[7]
    return p


def _identical():
    return np.tile(np.array([[0.375, -1.25, 2.5]]), (200, 1))


def _flat():
    p = np.random.default_rng(3).random((500, 3))
    p[:, 2] = 0.625
    return p


def _collinear():
    t = np.random.default_rng(4).random(300)
    return np.array([0.5, -1.0, 2.0]) + t[:, None] * np.array([1.0, 0.5, -0.25])


def _clusters():
    rng = np.random.default_rng(5)
    return np.concatenate([rng.random((80, 3)), 1000.0 + rng.random((80, 3)), [[500.0, 300.0, 200.0]]])


def _shifted_sphere():
    return 2.0 ** 20 + fibonacci_sphere(600) * 2.0 ** -20


def small(n, seed=6):
    return np.random.default_rng(seed).random((n, 3))


CLOUDS = {"uniform": _uniform, "lattice": _lattice, "duplicates": _duplicates, "identical": _identical, "flat": _flat, "collinear": _collinear,
          "clusters": _clusters, "shifted_sphere": _shifted_sphere, "one": lambda: small(1)}


@functools.lru_cache(maxsize=None)
def cloud(name):
    """the cloud and full_order of it as its own queries, computed once; read only"""
    p = np.ascontiguousarray(CLOUDS[name](), dtype=np.float64)
    ordered = full_order(p)
    for a in (p,) + ordered:
        a.setflags(write=False)
    return p, ordered


def separate_queries(points, seed=0):
    """queries that are not the points: 40 on points exactly, 100 inside the box, 24 about 100 extents outside it (on one axis and on all)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = max(float((hi - lo).max()), 1.0)
    on = p[rng.integers(0, len(p), 40)]
    inside = lo + rng.random((100, 3)) * (hi - lo)
    out = []
    for a in range(3):
        for sgn in (-1.0, 1.0):
            for _ in range(2):
                q = lo + rng.random(3) * (hi - lo)
                q[a] += sgn * 100.0 * ext
                out.append(q)
    out += [0.5 * (lo + hi) + 100.0 * ext * np.array(sg, dtype=np.float64) for sg in ((1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1)) for _ in range(3)]
    return np.concatenate([on, inside, np.array(out)])


@functools.lru_cache(maxsize=None)
def cloud_queries(name):
    p, _ = cloud(name)
    q = separate_queries(p, seed=len(name))
    ordered = full_order(p, q)
    for a in (q,) + ordered:
        a.setflags(write=False)
    return q, ordered
