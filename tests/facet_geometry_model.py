"""CPU model of the facet geometry columns of `<scene>_fgeom.npz` (the contract of dgnn_cell_circumspheres / dgnn_facet_geometry,
include/dgnn_hip.h): numpy in the header's OPERATION ORDER, so that the fp64 evaluation equals the device bit for bit; with
``np.longdouble`` the same expressions in extended precision.

* ``cell_circumspheres(vertices, tetrahedra)``: the per-cell pass, centre o = p0 + c and radius R = |c| of §23;
* ``facet_geometry(scene)``: the per-facet pass from the stored (o, R): area, cos_own, cos_neighbor, beta per directed row 4 t + k, and the
  stats.  The vector operations are graph_cut_weights_model's; its `_side` recomputes the sphere per facet row, this one loads it.
"""
from __future__ import annotations

import numpy as np

from graph_cut_weights_model import MalformedScene, _cross, _dot, _sub

FGEOM_KEYS = ("area", "cos_own", "cos_neighbor", "beta")


def cell_circumspheres(vertices, tetrahedra, dtype=np.float64):
    """-> dict(centre [T, 3], radius [T] in `dtype`, n_flat): a flat cell (det == 0) divides by zero, its radius is inf or NaN"""
    v = np.asarray(vertices, dtype=np.float64).astype(dtype).reshape(-1, 3)
    t = np.asarray(tetrahedra).astype(np.int64).reshape(-1, 4)
    if ((t < 0) | (t >= len(v))).any():
        raise MalformedScene("a vertex id of a cell out of range")
    p0 = v[t[:, 0]]
    u, vv, w = _sub(v[t[:, 1]], p0), _sub(v[t[:, 2]], p0), _sub(v[t[:, 3]], p0)
    vw, wu, uv = _cross(vv, w), _cross(w, u), _cross(u, vv)
    det = _dot(u, vw)
    u2, v2, w2 = _dot(u, u), _dot(vv, vv), _dot(w, w)
    d2 = 2 * det
    with np.errstate(all="ignore"):
        c = np.stack([((u2 * vw[:, k] + v2 * wu[:, k]) + w2 * uv[:, k]) / d2 for k in range(3)], axis=1).reshape(-1, 3)
        return dict(centre=(p0 + c).astype(dtype), radius=np.sqrt(_dot(c, c)).astype(dtype), n_flat=int((det == 0).sum()))


def _side_from_sphere(v, tets, cells, fac, a, n, nn, o, R):
    """(cos phi [m], neutral bool [m], slot [m]) of the facets `fac` [m, 3] seen from the cells `cells` [m] with the stored spheres (o, R)"""
    t = tets[cells]
    if ((t < 0) | (t >= len(v))).any():
        raise MalformedScene("a vertex id of a cell out of range")
    inside = (t[:, :, None] == fac[:, None, :]).any(axis=2)                     # [m, 4]: cell vertex k is one of the facet's
    has = (t[:, :, None] == fac[:, None, :]).any(axis=1).all(axis=1)            # each facet id is in the cell
    if not ((inside.sum(axis=1) == 3) & has).all():
        raise MalformedScene("a facet is not a face of the cell its nfacets row names")
    slot = np.argmin(inside, axis=1)
    d = v[t[np.arange(len(t)), slot]]
    with np.errstate(all="ignore"):
        sd = _dot(n, _sub(d, a))
        hn = _dot(n, _sub(o[cells], a))
        h = np.where(sd > 0, hn, -hn) / nn
        r = h / R[cells]
        neutral = (nn == 0) | (sd == 0) | ~np.isfinite(R[cells]) | ~np.isfinite(h) | ~np.isfinite(r)
        cos = np.where(neutral, 0, np.where(r < -1, -1, np.where(r > 1, 1, r)))
    return cos.astype(v.dtype), neutral, slot


def facet_geometry(scene, dtype=np.float64):
    """-> dict of the four FGEOM_KEYS columns [4 T] in `dtype` (0 in a row that no facet names) and "stats": rows written, rows whose
    neighbour is the infinite cell, neutral sides, flat cells.  MalformedScene for what the device reports as malformed input."""
    v = np.asarray(scene["vertices"], dtype=np.float64).astype(dtype).reshape(-1, 3)
    tets = np.asarray(scene["tetrahedra"]).astype(np.int64).reshape(-1, 4)
    facets = np.asarray(scene["facets"]).astype(np.int64).reshape(-1, 3)
    nfacets = np.asarray(scene["nfacets"]).astype(np.int64).reshape(-1, 2)
    if ((facets < 0) | (facets >= len(v))).any() or (nfacets >= len(tets)).any():
        raise MalformedScene("an id out of range")
    sph = cell_circumspheres(v, tets, dtype)
    out = {k: np.zeros(4 * len(tets), dtype=dtype) for k in FGEOM_KEYS}
    stats = dict(rows=0, hull_rows=0, neutral_sides=0, n_flat=sph["n_flat"])
    finite = nfacets >= 0
    live = np.nonzero(finite.any(axis=1))[0]
    if len(live) == 0:
        return dict(out, stats=stats, written=np.zeros(4 * len(tets), dtype=np.int64))
    fac, cells, fin = facets[live], nfacets[live], finite[live]
    a = v[fac[:, 0]]
    n = _cross(_sub(v[fac[:, 1]], a), _sub(v[fac[:, 2]], a))
    nn = np.sqrt(_dot(n, n))
    area = dtype(0.5) * nn
    cos = np.ones((len(live), 2), dtype=dtype)          # the infinite cell: 1.0, not counted as neutral
    slot = np.zeros((len(live), 2), dtype=np.int64)
    for s in (0, 1):
        m = fin[:, s]
        cos[m, s], neutral, slot[m, s] = _side_from_sphere(v, tets, cells[m, s], fac[m], a[m], n[m], nn[m], sph["centre"], sph["radius"])
        stats["neutral_sides"] += int(neutral.sum())
    beta = 1 - np.where(cos[:, 0] < cos[:, 1], cos[:, 0], cos[:, 1])
    written = np.zeros(4 * len(tets), dtype=np.int64)
    for s in (0, 1):
        m = fin[:, s]
        row = 4 * cells[m, s] + slot[m, s]
        np.add.at(written, row, 1)
        out["area"][row], out["cos_own"][row], out["cos_neighbor"][row], out["beta"][row] = area[m], cos[m, s], cos[m, 1 - s], beta[m]
        stats["rows"] += int(m.sum())
        stats["hull_rows"] += int((m & ~fin[:, 1 - s]).sum())
    return dict(out, stats=stats, written=written)


def single_tet_scene():
    """T = 1, F = 4, every facet on the hull"""
    t = [0, 1, 2, 3]
    return dict(vertices=np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64), tetrahedra=np.array([t], dtype=np.int32),
                facets=np.array([[t[j] for j in range(4) if j != k] for k in range(4)], dtype=np.int32),
                nfacets=np.array([[0, -1]] * 4, dtype=np.int32))


def facet_rows(scene):
    """int64 [F, 2]: the row 4 t + k of either side of every facet (-1 for the infinite side)"""
    tets = np.asarray(scene["tetrahedra"]).astype(np.int64)
    fac, nf = np.asarray(scene["facets"]).astype(np.int64), np.asarray(scene["nfacets"]).astype(np.int64)
    rows = np.full((len(fac), 2), -1, dtype=np.int64)
    for s in (0, 1):
        m = nf[:, s] >= 0
        inside = (tets[nf[m, s]][:, :, None] == fac[m][:, None, :]).any(axis=2)
        rows[m, s] = 4 * nf[m, s] + np.argmin(inside, axis=1)
    return rows
