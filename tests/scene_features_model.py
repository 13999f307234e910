"""CPU model of the scene front end (the contract of dgnn_tet_neighbors / dgnn_cell_geometry / dgnn_vertex_incidence / dgnn_vertex_rays,
DESIGN §25): numpy fp64 with the kernels' operation order, every product, sum, division and square root rounding on its own.

* neighbours: slot k of a tet is the cell across the facet opposite its vertex k (-1 = the infinite cell);
* geometry: circumradius, volume, longest / shortest edge per tet and the fixed-order column sums behind the loader's mean_edge;
* incidence: vertex -> (tet, slot) of the finite tets, each row sorted here (the device leaves the order inside a row open);
* vertex rays: per ray the `outside` and `inside` (tet, slot, dist), and the count / min / max / sum aggregates per tet and per
  (tet, slot).  The side decisions are exact: the fp64 filter of csrc/exact_orient.h, then `fractions.Fraction` on the floats' exact values.
"""
from __future__ import annotations

import glob
import os
from fractions import Fraction

import numpy as np

OUTSIDE, INSIDE = 0, 1
SIDES = ("outside", "inside")
CHUNK = 256          # csrc/fixed_sum.h
RAY_STATS = ("rays", "used", "duplicates", "degenerate", "no_outside", "no_inside", "exact_used")
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
OTHERS = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])          # the other three slots of a tet, in slot order


# ---- neighbours --------------------------------------------------------------------------------------------------------------------
def tet_neighbors(facets, nfacets, tetrahedra):
    """-> (neighbors int32 [T, 4], number of (facet, cell) pairs whose facet is not a face of the cell)"""
    fac, nf, tets = np.asarray(facets, np.int64), np.asarray(nfacets, np.int64), np.asarray(tetrahedra, np.int64)
    nbr = np.full((len(tets), 4), -1, dtype=np.int32)
    bad = 0
    for side in (0, 1):
        ids = np.nonzero(nf[:, side] >= 0)[0]
        c = nf[ids, side]
        hit = (tets[c][:, :, None] == fac[ids][:, None, :]).any(axis=2)          # [m, 4]: vertex k of the cell lies on the facet
        ok = hit.sum(axis=1) == 3
        bad += int((~ok).sum())
        nbr[c[ok], np.argmin(hit[ok], axis=1)] = nf[ids[ok], 1 - side]
    return nbr, bad


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def fixed_sum(x):
    """csrc/fixed_sum.h: serial sums of chunks of 256 from 0.0, then the chunk totals serially from 0.0"""
    x = np.asarray(x, np.float64)
    nch = (len(x) + CHUNK - 1) // CHUNK
    pad = np.zeros(nch * CHUNK)
    pad[:len(x)] = x
    pad = pad.reshape(nch, CHUNK)
    part = np.zeros(nch)
    for j in range(CHUNK):
        part = part + pad[:, j]
    total = 0.0
    for p in part:
        total = total + float(p)
    return total


def cell_geometry(vertices, tetrahedra):
    """-> dict(radius, vol, longest_edge, shortest_edge [T] fp64, n_flat, sum_longest, sum_shortest)"""
    v, tets = np.asarray(vertices, np.float64), np.asarray(tetrahedra, np.int64)
    p = [[v[tets[:, k], a] for a in range(3)] for k in range(4)]
    u, w1, w2 = ([p[k][a] - p[0][a] for a in range(3)] for k in (1, 2, 3))
    c_vw, c_wu, c_uv = _cross(w1, w2), _cross(w2, u), _cross(u, w1)
    det = _dot(u, c_vw)
    u2, v2, w2n = _dot(u, u), _dot(w1, w1), _dot(w2, w2)
    r = [(u2 * c_vw[a] + v2 * c_wu[a]) + w2n * c_uv[a] for a in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        radius = np.where(det == 0.0, np.inf, np.sqrt(_dot(r, r)) / (2.0 * np.abs(det)))
    lens = []
    for i, j in PAIRS:
        d = [p[j][a] - p[i][a] for a in range(3)]
        lens.append(np.sqrt(_dot(d, d)))
    lens = np.stack(lens, axis=1) if len(tets) else np.zeros((0, 6))
    longest, shortest = lens.max(axis=1), lens.min(axis=1)
    return dict(radius=radius, vol=np.abs(det) / 6.0, longest_edge=longest, shortest_edge=shortest, n_flat=int((det == 0.0).sum()),
                sum_longest=fixed_sum(longest), sum_shortest=fixed_sum(shortest))


def mean_edge(geom, n_cells):
    """the loader's mean_edge (processing/data.py) over `n_cells` cell rows, the infinite ones holding 0"""
    return (geom["sum_longest"] + geom["sum_shortest"]) / (2 * n_cells)


# ---- incidence ---------------------------------------------------------------------------------------------------------------------
def vertex_incidence(tetrahedra, n_vertices):
    """-> (rowptr int32 [V + 1], entries int32 [4 T] = 4 * tet + slot, ascending inside a row)"""
    tets = np.asarray(tetrahedra, np.int64).reshape(-1)
    order = np.argsort(tets, kind="stable")
    rowptr = np.zeros(n_vertices + 1, dtype=np.int64)
    np.cumsum(np.bincount(tets, minlength=n_vertices), out=rowptr[1:])
    return rowptr.astype(np.int32), order.astype(np.int32)


# ---- exact orientation -------------------------------------------------------------------------------------------------------------
def _orient_exact(a, b, c, p):
    r = [[Fraction(float(x[i])) - Fraction(float(a[i])) for i in range(3)] for x in (b, c, p)]
    d = (r[0][0] * (r[1][1] * r[2][2] - r[1][2] * r[2][1]) - r[0][1] * (r[1][0] * r[2][2] - r[1][2] * r[2][0])
         + r[0][2] * (r[1][0] * r[2][1] - r[1][1] * r[2][0]))
    return (d > 0) - (d < 0)


def orient_sign(a, b, c, p):
    """exact sign of det[b - a, c - a, p - a], rows [n, 3] -> (int8 [n], number decided by the exact stage)"""
    ux, uy, uz = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], b[:, 2] - a[:, 2]
    vx, vy, vz = c[:, 0] - a[:, 0], c[:, 1] - a[:, 1], c[:, 2] - a[:, 2]
    wx, wy, wz = p[:, 0] - a[:, 0], p[:, 1] - a[:, 1], p[:, 2] - a[:, 2]
    m0, m1, m2, m3, m4, m5 = vy * wz, vz * wy, vx * wz, vz * wx, vx * wy, vy * wx
    det = ux * (m0 - m1) - uy * (m2 - m3) + uz * (m4 - m5)
    perm = np.abs(ux) * (np.abs(m0) + np.abs(m1)) + np.abs(uy) * (np.abs(m2) + np.abs(m3)) + np.abs(uz) * (np.abs(m4) + np.abs(m5))
    bound = (7.0 + 56.0 * 2.0 ** -53) * 2.0 ** -53 * perm + 2.0 ** -700
    sign = np.where(det > bound, 1, np.where(-det > bound, -1, 0)).astype(np.int8)
    hard = np.nonzero((det <= bound) & (-det <= bound))[0]
    for i in hard:
        sign[i] = _orient_exact(a[i], b[i], c[i], p[i])
    return sign, len(hard)


# ---- vertex rays -------------------------------------------------------------------------------------------------------------------
def first_rays(ray_vertex, n_vertices):
    """mask of the lowest-index ray of every vertex"""
    rv = np.asarray(ray_vertex, np.int64)
    first = np.full(n_vertices, len(rv), dtype=np.int64)
    np.minimum.at(first, rv, np.arange(len(rv)))
    return first[rv] == np.arange(len(rv))


def vertex_rays(vertices, tetrahedra, ray_vertex, sensors, unique=True):
    """-> dict: ray_tet, ray_slot int32 [R, 2] (-1 = none; column 0 outside, 1 inside), ray_dist fp64 [R, 2] (0 where none),
    per side s in SIDES: <s>_tet_{count,min,max,sum} [T], <s>_slot_{count,min,max,sum} [T, 4]; stats: dict of RAY_STATS"""
    v, tets = np.asarray(vertices, np.float64), np.asarray(tetrahedra, np.int64)
    rv, s = np.asarray(ray_vertex, np.int64).reshape(-1), np.asarray(sensors, np.float64).reshape(-1, 3)
    n_r, n_t = len(rv), len(tets)
    rowptr, entries = vertex_incidence(tets, len(v))
    p = v[rv]
    degenerate = (s == p).all(axis=1)
    dup = ~first_rays(rv, len(v)) if unique else np.zeros(n_r, dtype=bool)
    live = ~degenerate & ~dup
    # every (live ray, incident tet) pair
    deg = (rowptr[rv + 1] - rowptr[rv]) * live
    ray = np.repeat(np.arange(n_r), deg)
    off = np.arange(len(ray)) - np.repeat(np.cumsum(deg) - deg, deg)
    ent = entries[rowptr[rv[ray]] + off].astype(np.int64)
    t, k = ent // 4, ent % 4
    q = [v[tets[t, OTHERS[k, j]]] for j in range(3)]
    pp, ss = p[ray], s[ray]
    d_sign, n_exact = orient_sign(pp, q[0], q[1], q[2])
    exact = n_exact
    sg = []
    for a, b in ((0, 1), (1, 2), (2, 0)):
        g, n_exact = orient_sign(pp, q[a], q[b], ss)
        sg.append(g.astype(np.int64) * d_sign)
        exact += n_exact
    sg = np.stack(sg, axis=1) if len(ray) else np.zeros((0, 3), dtype=np.int64)
    ok = [(d_sign != 0) & (sg >= 0).all(axis=1), (d_sign != 0) & (sg <= 0).all(axis=1)]

    ray_tet = np.full((n_r, 2), -1, dtype=np.int32)
    ray_slot = np.full((n_r, 2), -1, dtype=np.int32)
    ray_dist = np.zeros((n_r, 2))
    for side in (OUTSIDE, INSIDE):
        sel = np.nonzero(ok[side])[0]
        sel = sel[np.lexsort((t[sel], ray[sel]))]                                   # by ray, then by tet: the first of a ray is its lowest tet
        sel = sel[np.r_[True, ray[sel][1:] != ray[sel][:-1]]] if len(sel) else sel
        r_ = ray[sel]
        ray_tet[r_, side], ray_slot[r_, side] = t[sel], k[sel]
        e = [ss[sel, a] - pp[sel, a] for a in range(3)]
        ln = np.sqrt(_dot(e, e))
        d = [e[a] / ln for a in range(3)]
        if side == INSIDE:
            d = [-x for x in d]
        q0, q1, q2 = (q[j][sel] for j in range(3))
        n = _cross([q1[:, a] - q0[:, a] for a in range(3)], [q2[:, a] - q0[:, a] for a in range(3)])
        w = [q0[:, a] - pp[sel, a] for a in range(3)]
        with np.errstate(divide="ignore", invalid="ignore"):
            ray_dist[r_, side] = _dot(n, w) / _dot(n, d)

    out = dict(ray_tet=ray_tet, ray_slot=ray_slot, ray_dist=ray_dist)
    for side, name in enumerate(SIDES):
        agg = {"tet": (np.zeros(n_t, np.int32), np.zeros(n_t), np.zeros(n_t), np.zeros(n_t)),
               "slot": (np.zeros((n_t, 4), np.int32), np.zeros((n_t, 4)), np.zeros((n_t, 4)), np.zeros((n_t, 4)))}
        for r in np.nonzero(ray_tet[:, side] >= 0)[0]:                              # ascending ray index: the order of the sums
            tt, kk, dd = int(ray_tet[r, side]), int(ray_slot[r, side]), ray_dist[r, side]
            for (cnt, lo, hi, sm), idx in ((agg["tet"], tt), (agg["slot"], (tt, kk))):
                lo[idx] = dd if cnt[idx] == 0 else min(lo[idx], dd)
                hi[idx] = dd if cnt[idx] == 0 else max(hi[idx], dd)
                sm[idx] = sm[idx] + dd
                cnt[idx] += 1
        for level in ("tet", "slot"):
            for stat, a in zip(("count", "min", "max", "sum"), agg[level]):
                out["%s_%s_%s" % (name, level, stat)] = a
    out["stats"] = dict(rays=n_r, used=int(live.sum()), duplicates=int((dup & ~degenerate).sum()), degenerate=int(degenerate.sum()),
                        no_outside=int((live & (ray_tet[:, 0] < 0)).sum()), no_inside=int((live & (ray_tet[:, 1] < 0)).sum()), exact_used=exact)
    return out


# ---- the scene files ---------------------------------------------------------------------------------------------------------------
def match_vertices(vertices, points):
    """-> vertex id of every point by exact coordinate match (-1 = none; the lowest id among equal vertices)"""
    v, pts = np.ascontiguousarray(vertices, np.float64), np.ascontiguousarray(points, np.float64)
    key = lambda x: (x + 0.0).view(np.dtype((np.void, 24))).reshape(-1)          # (+ 0.0: -0.0 and 0.0 are one coordinate)
    kv, kp = key(v), key(pts)
    order = np.argsort(kv, kind="stable")
    pos = np.searchsorted(kv[order], kp)
    pos = np.minimum(pos, len(v) - 1)
    return np.where(kv[order][pos] == kp, order[pos], -1).astype(np.int64)


def cell_rows(infinite):
    """-> (cell id of every finite tet, tet id of every cell or -1)"""
    inf = np.asarray(infinite).astype(bool)
    cell_of_tet = np.nonzero(~inf)[0]
    tet_of_cell = np.full(len(inf), -1, dtype=np.int64)
    tet_of_cell[cell_of_tet] = np.arange(len(cell_of_tet))
    return cell_of_tet, tet_of_cell


def scene_columns(geom, rays, infinite):
    """the model's cgeom / cbvf / fbvf columns in cell rows and edge rows 4 c + k (the non-`last` ones)"""
    cell_of_tet, _ = cell_rows(infinite)
    n = len(infinite)
    out = {}
    for key in ("radius", "vol", "longest_edge", "shortest_edge"):
        col = np.zeros(n)
        col[cell_of_tet] = geom[key]
        out[key] = col
    for side in ("inside", "outside"):
        for stat in ("count", "min", "max", "sum"):
            name = "vertex_%s_%s" % (side, stat if stat == "count" else "dist_" + stat)
            col = np.zeros(n)
            col[cell_of_tet] = rays["%s_tet_%s" % (side, stat)]
            out["cb_" + name] = col
            col = np.zeros((n, 4))
            col[cell_of_tet] = rays["%s_slot_%s" % (side, stat)]
            out["fb_" + name] = col.reshape(-1)
    return out


# ---- the recorded files of Ignatius scene 99 (tests/golden/make_golden_scene_features.py) ---------------------------------------------------
FIXTURE_STEM = "ignatius_scene_features"
DIST_RTOL, DIST_FLOOR = 1e-12, 1e-3          # |ours - recorded| <= 1e-12 * max(|recorded|, 1e-3): measured max |d| 8.5e-16
GEOM_RTOL = 1e-10                            # vol / radius: measured 2.9e-12 (profiles/scene_features.md); the margin covers another summation order


def load_fixture(folder=os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")):
    """every part of the fixture as one dict"""
    out = {}
    for path in sorted(glob.glob(os.path.join(folder, FIXTURE_STEM + "*.npz"))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def recorded_columns(fx):
    """the recorded cgeom / cbvf / fbvf columns in full rows, in file order (the sparse columns of the fixture scattered back)"""
    rec = {k: fx[k] for k in ("radius", "vol", "longest_edge", "shortest_edge")}
    for pre in ("cb", "fb"):
        n = int(fx[pre + "_rows_total"])
        for k in fx["vf_keys_" + pre]:
            k = str(k)
            col = np.zeros(n)
            if "_last_" not in k:
                col[fx["%s_%s_rows" % (pre, k.split("_")[2])]] = fx[k]
            rec[k] = col
    return rec


def check_against_recorded(cols, rec):
    """the bounds the recorded files set, for any producer of the columns: the model and the device"""
    for k in ("longest_edge", "shortest_edge"):
        assert np.array_equal(cols[k], rec[k]), k
    for k in ("vol", "radius"):
        rel = np.abs(cols[k] - rec[k]) / np.where(rec[k] != 0, np.abs(rec[k]), 1.0)
        print("%s: max relative error %.3g" % (k, rel.max()))
        assert (rel <= GEOM_RTOL).all() and np.array_equal(cols[k] == 0, rec[k] == 0), k
    for pre in ("cb", "fb"):
        for side in ("inside", "outside"):
            k = "%s_vertex_%s_count" % (pre, side)
            assert np.array_equal(cols[k], rec[k]), k
            for stat in ("dist_min", "dist_max", "dist_sum"):
                k = "%s_vertex_%s_%s" % (pre, side, stat)
                d = np.abs(cols[k] - rec[k])
                print("%s: max |d| %.3g" % (k, d.max()))
                assert (d <= DIST_RTOL * np.maximum(np.abs(rec[k]), DIST_FLOOR)).all(), k


# ---- hand-made scenes --------------------------------------------------------------------------------------------------------------
def facets_from_tets(tetrahedra):
    """-> (facets int32 [F, 3], nfacets int32 [F, 2]): every face of the tets once, with its one or two cells (-1 = the infinite cell)"""
    tets = np.asarray(tetrahedra, np.int64)
    faces = np.sort(np.concatenate([tets[:, OTHERS[k]] for k in range(4)]), axis=1)
    cell = np.tile(np.arange(len(tets)), 4)
    uniq, inv, cnt = np.unique(faces, axis=0, return_inverse=True, return_counts=True)
    assert cnt.max() <= 2
    nf = np.full((len(uniq), 2), -1, dtype=np.int32)
    for c, f in sorted(zip(cell.tolist(), inv.reshape(-1).tolist())):
        nf[f, 0 if nf[f, 0] < 0 else 1] = c
    return uniq.astype(np.int32), nf
