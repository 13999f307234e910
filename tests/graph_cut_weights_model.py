"""CPU model of the per-facet graph-cut weights and of the weighted cut (the contract of dgnn_facet_cut_terms / dgnn_graph_cut_weighted,
include/dgnn_hip.h).

* ``facet_terms(scene, kind, dtype)``: q_f of every facet of a `_3dt.npz` scene in numpy, in the header's OPERATION ORDER, so that the
  fp64 evaluation equals the device bit for bit; with ``np.longdouble`` the same expressions in extended precision (the yardstick of the
  fp64 rounding);
* ``quantise``: w_f = rint(binary_weight * q_f), half to even;
* ``brute_force_weighted`` (n <= 14) and ``solve_weighted``: graph_cut_model's oracles with one capacity per row.
"""
from __future__ import annotations

import numpy as np

import graph_cut_model as gcm

SUM_CHUNK = 256
KINDS = ("area", "beta")


# ---- the header's vector operations ----------------------------------------------------------------------------------------------
def _sub(x, y):
    return x - y


def _cross(x, y):
    return np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], axis=1)


def _dot(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


def fixed_sum(x):
    """the sum of x in the device's order: serial inside chunks of 256 consecutive elements, the chunk sums then serially in chunk order"""
    x = np.asarray(x)
    n = len(x)
    nch = -(-n // SUM_CHUNK)
    pad = np.zeros(nch * SUM_CHUNK, dtype=x.dtype)      # x + 0.0 == x: the padding of the last chunk changes nothing
    pad[:n] = x
    pad = pad.reshape(nch, SUM_CHUNK)
    part = np.zeros(nch, dtype=x.dtype)
    for k in range(SUM_CHUNK):
        part = part + pad[:, k]
    total = x.dtype.type(0)
    for t in range(nch):
        total = total + part[t]
    return total


def graph_rows(nfacets):
    """bool [F]: the facets between two finite cells (reference generate_mesh.py:86-87)"""
    return (np.asarray(nfacets) >= 0).all(axis=1)


class MalformedScene(ValueError):
    pass


def _side(v, tets, cells, fac, a, n, nn):
    """(cos phi [m], neutral bool [m]) of the facets `fac` [m, 3] seen from the cells `cells` [m]"""
    t = tets[cells].astype(np.int64)
    if ((t < 0) | (t >= len(v))).any():
        raise MalformedScene("a vertex id of a cell out of range")
    inside = (t[:, :, None] == fac[:, None, :]).any(axis=2)                     # [m, 4]: cell vertex k is one of the facet's
    has = (t[:, :, None] == fac[:, None, :]).any(axis=1).all(axis=1)            # each facet id is in the cell
    if not ((inside.sum(axis=1) == 3) & has).all():
        raise MalformedScene("a facet is not a face of the cell its nfacets row names")
    opp = t[np.arange(len(t)), np.argmin(inside, axis=1)]
    p0 = v[t[:, 0]]
    u, vv, w = _sub(v[t[:, 1]], p0), _sub(v[t[:, 2]], p0), _sub(v[t[:, 3]], p0)
    vw, wu, uv = _cross(vv, w), _cross(w, u), _cross(u, vv)
    det = _dot(u, vw)
    u2, v2, w2 = _dot(u, u), _dot(vv, vv), _dot(w, w)
    d2 = 2 * det
    with np.errstate(all="ignore"):
        c = np.stack([((u2 * vw[:, k] + v2 * wu[:, k]) + w2 * uv[:, k]) / d2 for k in range(3)], axis=1)
        R = np.sqrt(_dot(c, c))
        sd = _dot(n, _sub(v[opp], a))
        g = _sub(p0 + c, a)
        hn = _dot(n, g)
        h = np.where(sd > 0, hn, -hn) / nn
        r = h / R
        neutral = (det == 0) | (nn == 0) | (sd == 0) | ~np.isfinite(R) | ~np.isfinite(h) | ~np.isfinite(r)
        cos = np.where(neutral, 0, np.minimum(np.maximum(r, -1), 1))
    return cos.astype(v.dtype), neutral


def facet_terms(scene, kind, dtype=np.float64, return_stats=False):
    """q [F] in `dtype` (0 for a facet with an infinite cell); with return_stats also {"rows", "neutral_sides"}.  MalformedScene for what the
    device reports as malformed input, ZeroDivisionError for a mean area that is 0 or not finite."""
    assert kind in KINDS
    v = np.asarray(scene["vertices"], dtype=np.float64).astype(dtype)
    tets = np.asarray(scene["tetrahedra"]).astype(np.int64)
    facets = np.asarray(scene["facets"]).astype(np.int64)
    nfacets = np.asarray(scene["nfacets"]).astype(np.int64)
    if ((facets < 0) | (facets >= len(v))).any() or (nfacets >= len(tets)).any():
        raise MalformedScene("an id out of range")
    rows = graph_rows(nfacets)
    q = np.zeros(len(facets), dtype=dtype)
    stats = {"rows": int(rows.sum()), "neutral_sides": 0}
    if rows.any():
        fac = facets[rows]
        a = v[fac[:, 0]]
        n = _cross(_sub(v[fac[:, 1]], a), _sub(v[fac[:, 2]], a))
        nn = np.sqrt(_dot(n, n))
        if kind == "area":
            area = np.zeros(len(facets), dtype=dtype)
            area[rows] = dtype(0.5) * nn
            with np.errstate(all="ignore"):
                mean = fixed_sum(area) / dtype(stats["rows"])
            if not (mean > 0 and np.isfinite(mean)):
                raise ZeroDivisionError("the mean facet area is 0 or not finite")
            q[rows] = area[rows] / mean
        else:
            cos0, n0 = _side(v, tets, nfacets[rows, 0], fac, a, n, nn)
            cos1, n1 = _side(v, tets, nfacets[rows, 1], fac, a, n, nn)
            stats["neutral_sides"] = int(n0.sum() + n1.sum())
            q[rows] = 1 - np.where(cos0 < cos1, cos0, cos1)
    return (q, stats) if return_stats else q


def quantise(q, binary_weight):
    """w = rint(binary_weight * q) (the product in q's precision, half to even) as int64; ValueError when a weight reaches 2^30"""
    q = np.asarray(q)
    x = np.rint(q.dtype.type(binary_weight) * q)
    if not ((x >= 0) & (x < 2 ** 30)).all():
        raise ValueError("a weight is not in [0, 2^30)")
    return x.astype(np.int64)


# ---- the weighted cut ---------------------------------------------------------------------------------------------------------------
def energy_weighted(labels, D, edges, weights) -> int:
    labels = np.asarray(labels).astype(np.int64)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    weights = np.asarray(weights, dtype=np.int64)
    unary = int(D[np.arange(len(labels)), labels].sum())
    return unary + int((weights * (labels[edges[:, 0]] != labels[edges[:, 1]])).sum())


def brute_force_weighted(prediction, edges, unary_weight, weights):
    """-> (labels int32 [n], energy): every labelling, the least energy, then the fewest outside cells"""
    D = gcm.unary_costs(prediction, unary_weight)
    n = D.shape[0]
    assert n <= 14
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    weights = np.asarray(weights, dtype=np.int64).reshape(-1)
    assert len(weights) == len(edges) and (weights >= 0).all()
    L = (np.arange(1 << n, dtype=np.int64)[:, None] >> np.arange(n)) & 1          # [2^n, n]
    E = D[np.arange(n), L].sum(1) + ((L[:, edges[:, 0]] != L[:, edges[:, 1]]) * weights).sum(1)
    best = E.min()
    cand = np.nonzero(E == best)[0]
    ones = L[cand].sum(1)
    pick = cand[ones == ones.min()]
    assert len(pick) == 1, "the minimiser with the fewest outside cells is unique"
    return L[pick[0]].astype(np.int32), int(best)


def solve_weighted(prediction, edges, unary_weight, weights):
    """graph_cut_model.solve with caps = w_r per row -> (labels int32 [n], energy, flow)"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import breadth_first_order, maximum_flow

    D = gcm.unary_costs(prediction, unary_weight)
    n = D.shape[0]
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    weights = np.asarray(weights, dtype=np.int64).reshape(-1)
    assert len(weights) == len(edges) and (weights >= 0).all()
    s, t = n, n + 1
    cs = np.maximum(D[:, 1] - D[:, 0], 0)
    ct = np.maximum(D[:, 0] - D[:, 1], 0)
    real = edges[:, 0] != edges[:, 1]
    e, we = edges[real], weights[real]
    nodes = np.arange(n)
    rows = np.concatenate([np.full(n, s), nodes, e[:, 0], e[:, 1]])
    cols = np.concatenate([nodes, np.full(n, t), e[:, 1], e[:, 0]])
    caps = np.concatenate([cs, ct, we, we])
    keep = caps > 0
    # every arc with its reverse present (capacity 0 where there is none), duplicates summed
    r2 = np.concatenate([rows[keep], cols[keep]])
    c2 = np.concatenate([cols[keep], rows[keep]])
    v2 = np.concatenate([caps[keep], np.zeros(int(keep.sum()), dtype=np.int64)])
    assert v2.sum() < 2 ** 31 if len(v2) else True
    C = sp.csr_matrix((v2.astype(np.int32), (r2, c2)), shape=(n + 2, n + 2))
    C.sum_duplicates()
    res = maximum_flow(C, s, t, method="dinic")
    F = res.flow if hasattr(res, "flow") else res.residual
    R = (C.astype(np.int64) - F.astype(np.int64)).tocsr()
    R.data[R.data < 0] = 0
    R.eliminate_zeros()
    reach = breadth_first_order(R.T.tocsr(), t, directed=True, return_predecessors=False)
    labels = np.zeros(n, dtype=np.int32)
    labels[reach[reach < n]] = 1
    E = energy_weighted(labels, D, edges, weights)
    flow = int(res.flow_value)
    assert E == flow + int(np.minimum(D[:, 0], D[:, 1]).sum()), "max-flow / min-cut identity"
    return labels, E, flow


# ---- hand-made scenes -----------------------------------------------------------------------------------------------------------------
def two_cell_scene(points, cells=((0, 1, 2, 3), (0, 1, 2, 4)), shared=(0, 1, 2)):
    """two cells on the common face `shared`: one finite-finite facet (row 0) and the six hull facets"""
    tets = np.asarray(cells, dtype=np.int32)
    facets, nfacets = [list(shared)], [[0, 1]]
    for c, t in enumerate(cells):
        for k in range(4):
            f = [t[j] for j in range(4) if j != k]
            if sorted(f) != sorted(shared):
                facets.append(f)
                nfacets.append([c, -1])
    return dict(vertices=np.asarray(points, dtype=np.float64), tetrahedra=tets, facets=np.asarray(facets, dtype=np.int32),
                nfacets=np.asarray(nfacets, dtype=np.int32))


def regular_pair_scene():
    """two regular tetrahedra of edge 1 on a common face: q_beta = 2/3 at that face"""
    h = np.sqrt(2.0 / 3.0)
    base = [[0, 0, 0], [1, 0, 0], [0.5, np.sqrt(3.0) / 2, 0]]
    g = [0.5, np.sqrt(3.0) / 6, 0]
    return two_cell_scene(base + [[g[0], g[1], h], [g[0], g[1], -h]])


def corner_scene(face):
    """the corner cell (0,0,0),(1,0,0),(0,1,0),(0,0,1) and its mirror image across `face` ("z0": the face z = 0, "diag": x + y + z = 1): both
    sides of the shared facet see the same cosine, 1/sqrt(3) resp. -1/3"""
    p = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    if face == "z0":
        return two_cell_scene(p + [[0, 0, -1]], cells=((0, 1, 2, 3), (0, 1, 2, 4)), shared=(0, 1, 2))
    return two_cell_scene(p + [[2.0 / 3, 2.0 / 3, 2.0 / 3]], cells=((0, 1, 2, 3), (4, 1, 2, 3)), shared=(1, 2, 3))


def degenerate_scene():
    """five cells; cell 1 is flat (its four vertices lie in z = 0) and the facet between cells 3 and 4 has no area (its vertices 6, 7, 8 are
    collinear).  Graph rows: facets 0 (cells 0, 1), 1 (cells 1, 2) and 2 (cells 3, 4); facets 3 and 4 are hull facets.  Neutral sides: cell
    1's side of rows 0 and 1, and both sides of row 2 (nn = 0) = 4.  Areas 0.5, 0.5, 0: mean 1/3."""
    v = [[0, 0, 1], [0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0],          # cell 0 = (0,1,2,3) on top of the flat cell 1 = (1,2,3,4)
         [1, 1, -1],                                                      # cell 2 = (2,3,4,5)
         [2, 0, 0], [3, 0, 0], [4, 0, 0], [2, 1, 1], [2, 1, -1]]          # cells 3 = (6,7,8,9) and 4 = (6,7,8,10) share the line 6-7-8
    tets = [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5], [6, 7, 8, 9], [6, 7, 8, 10]]
    facets = [[1, 2, 3], [2, 3, 4], [6, 7, 8], [0, 1, 2], [3, 4, 5]]
    nfacets = [[0, 1], [1, 2], [3, 4], [0, -1], [2, -1]]
    return dict(vertices=np.asarray(v, dtype=np.float64), tetrahedra=np.asarray(tets, dtype=np.int32), facets=np.asarray(facets, dtype=np.int32),
                nfacets=np.asarray(nfacets, dtype=np.int32))
