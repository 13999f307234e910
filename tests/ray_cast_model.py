"""CPU model of the first-hit ray caster and of the virtual scanner built on it (the contract of dgnn_ray_first_hit, include/dgnn_hip.h,
and of dgnn_amd/processing/scan_mesh.py): numpy fp64 with the kernel's operation order, every product, sum and division
rounding on its own.

* first hit: ALL PAIRS of (ray, face), chunked over the rays: no grid at all, so it states what the answer is whatever the binning.  The
  three signs of a pair come from the fp64 filter of csrc/exact_orient.h, vectorised, and from scene_features_model.orient_sign
  (`fractions.Fraction` on the floats' exact values) where the filter cannot decide;
* scanner: camera_positions and the composition of scan_mesh, given the aims (the device's area-uniform surface samples, which need the
  device's cumulative areas: the tests pass them in, the CPU checks draw them with mesh_metrics_model.sample).
"""
from __future__ import annotations

import numpy as np

import mesh_contains_model as mc
import scene_features_model as sf
from mesh_metrics_model import mm_hash

HIT_STATS = ("hits", "skipped", "degenerate", "exact_used")
SCAN_STATS = ("rays", "hits", "misses", "other_face", "degenerate", "exact_used")
SCAN_KEYS = ("points", "normals", "gt_normals", "sensor_position", "cameras", "noise", "outliers")


# ---- the signs -------------------------------------------------------------------------------------------------------------------
def orient_signs(a, b, c, p):
    """exact sign of det[b - a, c - a, p - a] for rows [n, 3] -> (int8 [n], bool [n]: decided by the exact stage)"""
    ux, uy, uz = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], b[:, 2] - a[:, 2]
    vx, vy, vz = c[:, 0] - a[:, 0], c[:, 1] - a[:, 1], c[:, 2] - a[:, 2]
    wx, wy, wz = p[:, 0] - a[:, 0], p[:, 1] - a[:, 1], p[:, 2] - a[:, 2]
    m0, m1, m2, m3, m4, m5 = vy * wz, vz * wy, vx * wz, vz * wx, vx * wy, vy * wx
    det = ux * (m0 - m1) - uy * (m2 - m3) + uz * (m4 - m5)
    perm = np.abs(ux) * (np.abs(m0) + np.abs(m1)) + np.abs(uy) * (np.abs(m2) + np.abs(m3)) + np.abs(uz) * (np.abs(m4) + np.abs(m5))
    bound = (7.0 + 56.0 * 2.0 ** -53) * 2.0 ** -53 * perm + 2.0 ** -700
    sign = np.where(det > bound, 1, np.where(-det > bound, -1, 0)).astype(np.int8)
    hard = ~((det > bound) | (-det > bound))
    idx = np.nonzero(hard)[0]
    if len(idx):
        sign[idx], n_exact = sf.orient_sign(a[idx], b[idx], c[idx], p[idx])
        assert n_exact == len(idx)          # the same filter: what it leaves open here, it leaves open there
    return sign, hard


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


# ---- first hit -------------------------------------------------------------------------------------------------------------------
def first_hit(vertices, faces, origins, aims, t_min=0.0, chunk=512):
    """-> (face int32 [n] (-1 = none), t fp64 [n] (0 where none), point fp64 [n, 3] (zeros where none), stats dict of HIT_STATS)"""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    o_all = np.asarray(origins).astype(np.float64).reshape(-1, 3)
    g_all = np.asarray(aims).astype(np.float64).reshape(-1, 3)
    n, nf = len(o_all), len(f)
    face = np.full(n, -1, dtype=np.int32)
    t_out = np.zeros(n)
    exact_of_hit = np.zeros(n, dtype=np.int64)
    skipped = (o_all == g_all).all(axis=1)
    degenerate = 0
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    nrm = _cross(b - a, c - a)                                                  # [F, 3]
    live = np.nonzero(~skipped)[0]
    for s in range(0, len(live), chunk):
        rows = live[s:s + chunk]
        m = len(rows)
        o, g = o_all[rows], g_all[rows]
        d = g - o
        rep = lambda x: np.repeat(x, nf, axis=0)                                 # ray-major pairs
        til = lambda x: np.tile(x, (m, 1))
        oo, gg = rep(o), rep(g)
        aa, bb, cc = til(a), til(b), til(c)
        s1, h1 = orient_signs(oo, gg, aa, bb)
        s2, h2 = orient_signs(oo, gg, bb, cc)
        s3, h3 = orient_signs(oo, gg, cc, aa)
        sg = np.stack([s1, s2, s3], axis=1)
        nonneg, nonpos = (sg >= 0).all(axis=1), (sg <= 0).all(axis=1)
        cross = ((nonneg | nonpos) & ~(nonneg & nonpos)).reshape(m, nf)
        n_exact = (h1.astype(np.int64) + h2 + h3).reshape(m, nf)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            num = _dot(nrm[None], a[None] - o[:, None])                          # [m, F]
            den = _dot(nrm[None], d[:, None])
            t = num / den
        bad = cross & ((den == 0) | ~np.isfinite(t))
        degenerate += int(bad.sum())
        ok = cross & ~bad & (t > t_min)
        tt = np.where(ok, t, np.inf)
        j = tt.argmin(axis=1)                                                    # the first minimiser: the lowest face id among equal t
        hit = ok[np.arange(m), j]
        face[rows[hit]] = j[hit]
        t_out[rows[hit]] = t[np.arange(m), j][hit]
        exact_of_hit[rows[hit]] = n_exact[np.arange(m), j][hit]
    d_all = g_all - o_all
    m_all = t_out[:, None] * d_all
    point = np.where((face >= 0)[:, None], o_all + m_all, 0.0)
    stats = dict(hits=int((face >= 0).sum()), skipped=int(skipped.sum()), degenerate=degenerate, exact_used=int(exact_of_hit.sum()))
    return face, t_out, point, stats


def filter_only_first_hit(vertices, faces, origins, aims, t_min=0.0, chunk=512):
    """the fp64 rule alone, every undecided sign read as 0: the host line of tools/bench_scan_mesh.py (no Fractions, so its time is numpy's)"""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    o_all, g_all = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(aims, dtype=np.float64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    nrm = _cross(b - a, c - a)
    face, t_out = np.full(len(o_all), -1, dtype=np.int32), np.zeros(len(o_all))

    def sign(o, g, x, y):          # [m, 1, 3] against [1, F, 3]
        u, vv, w = g - o, x - o, y - o
        m0, m1, m2, m3, m4, m5 = vv[..., 1] * w[..., 2], vv[..., 2] * w[..., 1], vv[..., 0] * w[..., 2], vv[..., 2] * w[..., 0], vv[..., 0] * w[..., 1], vv[..., 1] * w[..., 0]
        det = u[..., 0] * (m0 - m1) - u[..., 1] * (m2 - m3) + u[..., 2] * (m4 - m5)
        perm = np.abs(u[..., 0]) * (np.abs(m0) + np.abs(m1)) + np.abs(u[..., 1]) * (np.abs(m2) + np.abs(m3)) + np.abs(u[..., 2]) * (np.abs(m4) + np.abs(m5))
        bound = (7.0 + 56.0 * 2.0 ** -53) * 2.0 ** -53 * perm + 2.0 ** -700
        return np.where(det > bound, 1, np.where(-det > bound, -1, 0))

    for s in range(0, len(o_all), chunk):
        o, g = o_all[s:s + chunk, None], g_all[s:s + chunk, None]
        sg = np.stack([sign(o, g, a[None], b[None]), sign(o, g, b[None], c[None]), sign(o, g, c[None], a[None])], axis=-1)
        nonneg, nonpos = (sg >= 0).all(axis=-1), (sg <= 0).all(axis=-1)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t = _dot(nrm[None], a[None] - o) / _dot(nrm[None], g - o)
        ok = (nonneg | nonpos) & ~(nonneg & nonpos) & np.isfinite(t) & (t > t_min)
        tt = np.where(ok, t, np.inf)
        j = tt.argmin(axis=1)
        hit = ok[np.arange(len(j)), j]
        face[s:s + chunk][hit] = j[hit]
        t_out[s:s + chunk][hit] = tt[np.arange(len(j)), j][hit]
    return face, t_out


# ---- the scanner -----------------------------------------------------------------------------------------------------------------
def _u01(h):
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def sub_seeds(seed):
    """s1 .. s5 = mm_hash(seed, 1 .. 5): aims, sensor choice, noise, outliers, the outliers' sensors"""
    return [int(x) for x in mm_hash(seed, np.arange(1, 6, dtype=np.uint64))]


def frame(vertices, faces):
    """-> (centre of the referenced vertices' box, half its diagonal)"""
    used = np.asarray(vertices, dtype=np.float64)[np.unique(np.asarray(faces, dtype=np.int64))]
    lo, hi = used.min(axis=0), used.max(axis=0)
    ext = hi - lo
    return 0.5 * (lo + hi), 0.5 * np.sqrt((ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2])


def camera_positions(vertices, faces, n_cameras, distance=2.0, seed=0):
    centre, radius = frame(vertices, faces)
    k = np.arange(n_cameras, dtype=np.uint64)
    z = 2.0 * _u01(mm_hash(seed, np.uint64(2) * k + np.uint64(1))) - 1.0
    phi = 6.283185307179586 * _u01(mm_hash(seed, np.uint64(2) * k + np.uint64(2)))
    rho = np.sqrt(1.0 - z * z)
    unit = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)
    return centre + (distance * radius) * unit


def sensor_ids(seed, n, n_cameras):
    return (mm_hash(seed, np.arange(1, n + 1, dtype=np.uint64)) % np.uint64(n_cameras)).astype(np.int64)


def scanner_rays(vertices, faces, n=4096, cameras=10, distance=2.0, seed=0):
    """the rays scan_mesh casts, with numpy's cumulative areas in place of the device's -> (origins, aims (fp32 values) fp64, aim faces, cameras)"""
    from mesh_metrics_model import face_areas, sample

    s1, s2 = sub_seeds(seed)[:2]
    ids = np.arange(len(faces))
    aims, aim_face = sample(vertices, faces, ids, np.cumsum(face_areas(vertices, faces, ids)), n, s1)
    cams = camera_positions(vertices, faces, cameras, distance, seed)
    return cams[sensor_ids(s2, n, cameras)], aims.astype(np.float64), aim_face, cams


def scan_mesh(vertices, faces, aims, aim_face, cameras, noise=0.0, outliers=0.0, seed=0):
    """The composition of processing.scan_mesh.scan_mesh after its first step: `aims` fp32 [n, 3] with their faces `aim_face`, `cameras`
    [C, 3] (camera_positions or the caller's sensors) -> dict of points, normals, gt_normals, sensor_position fp64 and stats."""
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    _, s2, s3, s4, s5 = sub_seeds(seed)
    cams = np.asarray(cameras, dtype=np.float64).reshape(-1, 3)
    g = np.asarray(aims).astype(np.float64)
    n = len(g)
    o = cams[sensor_ids(s2, n, len(cams))]
    face, _, point, st = first_hit(v, f, o, g)
    hit = face >= 0
    pts, sens = point[hit], o[hit]
    gt = mc.face_normals(v, f)[face[hit]]
    to_sensor = sens - pts
    flip = _dot(gt, to_sensor) < 0
    normals = np.where(flip[:, None], -gt, gt)
    stats = dict(rays=n, hits=int(hit.sum()), misses=int((~hit).sum()), other_face=int((face[hit] != np.asarray(aim_face)[hit]).sum()),
                 degenerate=st["degenerate"], exact_used=st["exact_used"])
    if noise > 0:
        pts = mc.jitter_points(pts, noise, s3)
    n_out = int(round(outliers * len(pts))) if outliers > 0 else 0
    if n_out:
        centre, radius = frame(v, f)
        extra = mc.box_points(n_out, 2.0 * radius, s4) + centre
        extra_sens = cams[sensor_ids(s5, n_out, len(cams))]
        e = extra_sens - extra
        ln = np.sqrt(_dot(e, e))
        pts, sens = np.concatenate([pts, extra]), np.concatenate([sens, extra_sens])
        normals, gt = np.concatenate([normals, e / ln[:, None]]), np.concatenate([gt, np.zeros((n_out, 3))])
    return dict(points=pts, normals=normals, gt_normals=gt, sensor_position=sens, stats=stats)
