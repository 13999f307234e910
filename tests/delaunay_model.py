"""CPU model of the Delaunay contract: numpy plus `fractions`, no grid, no schedule, no insertion order.

Predicates: an fp64 evaluation with a generous static error bound decides the clear cases; everything else is decided exactly -- in int64 when
all coordinates are small integers, with Fractions otherwise.  The bounds here are looser than the device's (32 eps and 16 eps times the
permanent, whatever the operation order): a looser filter only sends more cases to the exact stage.

  orient_signs(a, b, c, d)       sign det[b - a, c - a, d - a]
  insphere_signs(a, b, c, d, e)  +1: e strictly inside the sphere through a..d, 0: on it, -1: outside; 0 for flat a..d
  certificate(points, tetrahedra, neighbors, hull_facets)  -> list of violations (empty = the output of ops.delaunay is what it claims)
  canonical(tets)                the row and table order of ops.delaunay
"""
from __future__ import annotations

import itertools
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -53


def _frac_rows(*arrays):
    return [[[Fraction(float(x)) for x in row] for row in np.asarray(a, dtype=np.float64).reshape(-1, 3)] for a in arrays]


def _small_ints(*arrays):
    return all(np.all(np.asarray(a) == np.round(a)) and np.all(np.abs(a) <= 512) for a in arrays)


def _det3(r0, r1, r2):
    return (r0[0] * (r1[1] * r2[2] - r1[2] * r2[1]) - r0[1] * (r1[0] * r2[2] - r1[2] * r2[0]) + r0[2] * (r1[0] * r2[1] - r1[1] * r2[0]))


def _sgn(x):
    return (x > 0) - (x < 0)


def _orient_exact_one(a, b, c, d):
    return _sgn(_det3([b[i] - a[i] for i in range(3)], [c[i] - a[i] for i in range(3)], [d[i] - a[i] for i in range(3)]))


def _lifted_det(a, b, c, d, e):
    """det of the rows [p - e, |p - e|^2], p = a..d (equal to the 5x5 determinant L of the rows [x y z x^2+y^2+z^2 1]); any exact number type"""
    rows = []
    for p in (a, b, c, d):
        q = [p[i] - e[i] for i in range(3)]
        rows.append(q + [q[0] * q[0] + q[1] * q[1] + q[2] * q[2]])
    ra, rb, rc, rd = rows
    return (-ra[3] * _det3(rb[:3], rc[:3], rd[:3]) + rb[3] * _det3(ra[:3], rc[:3], rd[:3]) - rc[3] * _det3(ra[:3], rb[:3], rd[:3])
            + rd[3] * _det3(ra[:3], rb[:3], rc[:3]))


def orient_signs(a, b, c, d):
    a, b, c, d = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (a, b, c, d))
    n = max(len(x) for x in (a, b, c, d))
    a, b, c, d = (np.broadcast_to(x, (n, 3)) for x in (a, b, c, d))
    if _small_ints(a, b, c, d):
        ai, bi, ci, di = (x.astype(np.int64) for x in (a, b, c, d))
        u, v, w = bi - ai, ci - ai, di - ai
        return np.sign(u[:, 0] * (v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1]) - u[:, 1] * (v[:, 0] * w[:, 2] - v[:, 2] * w[:, 0])
                       + u[:, 2] * (v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0])).astype(np.int8)
    with np.errstate(all="ignore"):
        u, v, w = b - a, c - a, d - a
        m = [v[:, 1] * w[:, 2], v[:, 2] * w[:, 1], v[:, 0] * w[:, 2], v[:, 2] * w[:, 0], v[:, 0] * w[:, 1], v[:, 1] * w[:, 0]]
        det = u[:, 0] * (m[0] - m[1]) - u[:, 1] * (m[2] - m[3]) + u[:, 2] * (m[4] - m[5])
        perm = (np.abs(u[:, 0]) * (np.abs(m[0]) + np.abs(m[1])) + np.abs(u[:, 1]) * (np.abs(m[2]) + np.abs(m[3]))
                + np.abs(u[:, 2]) * (np.abs(m[4]) + np.abs(m[5])))
        bound = 16 * EPS * perm + 2.0 ** -600
        clear = np.isfinite(det) & np.isfinite(perm) & (np.abs(det) > bound)
    out = np.sign(det).astype(np.int8)
    for i in np.nonzero(~clear)[0]:
        fa, fb, fc, fd = (r[0] for r in _frac_rows(a[i], b[i], c[i], d[i]))
        out[i] = _orient_exact_one(fa, fb, fc, fd)
    return out


def insphere_signs(a, b, c, d, e):
    a, b, c, d, e = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (a, b, c, d, e))
    n = max(len(x) for x in (a, b, c, d, e))
    a, b, c, d, e = (np.broadcast_to(x, (n, 3)) for x in (a, b, c, d, e))
    o = orient_signs(a, b, c, d).astype(np.int64)
    if _small_ints(a, b, c, d, e):     # |L| < 2^58: exact in int64
        A, B, C, D, E = (x.astype(np.int64).T for x in (a, b, c, d, e))
        L = _lifted_det(A, B, C, D, E)
        return (-np.sign(L) * o).astype(np.int8)
    with np.errstate(all="ignore"):
        p = [x - e for x in (a, b, c, d)]
        lift = [q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] for q in p]

        def m2(i, j):
            x, y = p[i][:, 0] * p[j][:, 1], p[j][:, 0] * p[i][:, 1]
            return x - y, np.abs(x) + np.abs(y)

        (ab, pab), (bc, pbc), (cd, pcd), (da, pda), (ac, pac), (bd, pbd) = m2(0, 1), m2(1, 2), m2(2, 3), m2(3, 0), m2(0, 2), m2(1, 3)
        az, bz, cz, dz = (q[:, 2] for q in p)
        abc, bcd = az * bc - bz * ac + cz * ab, bz * cd - cz * bd + dz * bc
        cda, dab = cz * da + dz * ac + az * cd, dz * ab + az * bd + bz * da
        det = (lift[3] * abc - lift[2] * dab) + (lift[1] * cda - lift[0] * bcd)
        faz, fbz, fcz, fdz = np.abs(az), np.abs(bz), np.abs(cz), np.abs(dz)
        perm = ((pcd * fbz + pbd * fcz + pbc * fdz) * lift[0] + (pda * fcz + pac * fdz + pcd * faz) * lift[1]
                + (pab * fdz + pbd * faz + pda * fbz) * lift[2] + (pbc * faz + pac * fbz + pab * fcz) * lift[3])
        bound = 32 * EPS * perm + 2.0 ** -500
        clear = np.isfinite(det) & np.isfinite(perm) & (np.abs(det) > bound)
    s = np.sign(det).astype(np.int64)
    for i in np.nonzero(~clear & (o != 0))[0]:
        fa, fb, fc, fd, fe = (r[0] for r in _frac_rows(a[i], b[i], c[i], d[i], e[i]))
        s[i] = _sgn(_lifted_det(fa, fb, fc, fd, fe))
    return (-s * o).astype(np.int8)


def _parity(p):
    return sum(p[i] > p[j] for i in range(len(p)) for j in range(i + 1, len(p))) & 1


EVEN_PERMS = [p for p in itertools.permutations(range(4)) if _parity(p) == 0]


def canonical(tets):
    """every row as the lexicographically smallest of its 12 even permutations (smallest vertex first), rows sorted lexicographically"""
    t = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    rows = [min(tuple(int(r[i]) for i in p) for p in EVEN_PERMS) for r in t]
    return np.array(sorted(rows), dtype=np.int64).reshape(-1, 4)


def signed_volume6(points, tets):
    """sum of det[v1 - v0, v2 - v0, v3 - v0] over the cells, exact (a Fraction)"""
    P = _frac_rows(points)[0]
    return sum(_det3([P[r[1]][i] - P[r[0]][i] for i in range(3)], [P[r[2]][i] - P[r[0]][i] for i in range(3)],
                     [P[r[3]][i] - P[r[0]][i] for i in range(3)]) for r in np.asarray(tets))


def strictly_delaunay(points, tets, chunk=256):
    """(cells with a point strictly inside, cells with a further point ON the sphere, flat cells) over all (cell, point) pairs; the cells
    may have either orientation (a host triangulator's do)"""
    P = np.asarray(points, dtype=np.float64)
    t = np.asarray(tets, dtype=np.int64).reshape(-1, 4)
    o = orient_signs(P[t[:, 0]], P[t[:, 1]], P[t[:, 2]], P[t[:, 3]])
    inside = on = 0
    n = len(P)
    for lo in range(0, len(t), chunk):
        tt = t[lo:lo + chunk]
        m = len(tt)
        rep = [np.repeat(P[tt[:, k]], n, axis=0) for k in range(4)]
        s = insphere_signs(rep[0], rep[1], rep[2], rep[3], np.tile(P, (m, 1))).reshape(m, n)
        own = np.zeros((m, n), dtype=bool)
        own[np.repeat(np.arange(m), 4), tt.reshape(-1)] = True
        inside += int(((s > 0).any(axis=1)).sum())
        on += int((((s == 0) & ~own).any(axis=1)).sum())
    return inside, on, int((o == 0).sum())


FACET_OF_SLOT = ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))


def certificate(points, tetrahedra, neighbors, hull_facets, inside=None):
    """All exact.  Returns the list of violated clauses (strings); [] certifies the triangulation.  inside: the first count of
    strictly_delaunay(points, tetrahedra) when the caller has it already (the all-pairs test is the expensive clause)."""
    from dgnn_amd.synthetic import check_four_regular

    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(tetrahedra, dtype=np.int64).reshape(-1, 4)
    nb = np.asarray(neighbors, dtype=np.int64).reshape(-1, 4)
    hf = np.asarray(hull_facets, dtype=np.int64).reshape(-1, 3)
    T, H, n = len(t), len(hf), len(P)
    bad = []
    if len(nb) != T + H:
        return ["neighbors has %d rows for %d + %d cells" % (len(nb), T, H)]
    if t.min() < 0 or t.max() >= n or nb.min() < 0 or nb.max() >= T + H:
        return ["ids out of range"]
    if not np.array_equal(t, canonical(t)):
        bad.append("rows are not canonical / sorted")
    o = orient_signs(P[t[:, 0]], P[t[:, 1]], P[t[:, 2]], P[t[:, 3]])
    if np.any(o <= 0):
        bad.append("%d cells are not strictly positive" % int((o <= 0).sum()))
    # adjacency, slot by slot
    wrong = 0
    hull_seen = np.zeros(H, dtype=np.int64)
    expect_h = 0
    for c in range(T):
        for k in range(4):
            f = set(t[c, list(FACET_OF_SLOT[k])])
            m = nb[c, k]
            if m < T:
                back = [j for j in range(4) if nb[m, j] == c]
                wrong += not (len(back) == 1 and set(t[m, list(FACET_OF_SLOT[back[0]])]) == f and m != c)
            else:
                h = m - T
                hull_seen[h] += 1
                wrong += not (nb[m, 0] == c and set(hf[h]) == f and h == expect_h)      # infinite cells ordered by (finite cell, slot)
                expect_h += 1
    for h in range(H):
        for j in range(3):
            m = nb[T + h, j + 1]
            edge = set(hf[h]) - {hf[h, j]}
            if m < T:
                wrong += 1
                continue
            back = [i for i in range(3) if nb[m, i + 1] == T + h]
            wrong += not (len(back) == 1 and edge <= set(hf[m - T]) and set(hf[m - T]) - {hf[m - T, back[0]]} == edge and m != T + h)
    if wrong or np.any(hull_seen != 1):
        bad.append("%d adjacency slots are inconsistent" % (wrong + int((hull_seen != 1).sum())))
    adj = np.stack([np.repeat(np.arange(T + H), 4), nb.reshape(-1)], axis=1)
    if not check_four_regular(adj):
        bad.append("the adjacency is not 4-regular and symmetric")
    if len(np.unique(t)) != n:
        bad.append("%d of %d points are vertices" % (len(np.unique(t)), n))
    if inside is None:
        inside, _, _ = strictly_delaunay(P, t)
    if inside:
        bad.append("%d cells hold a point strictly inside their sphere" % inside)
    front = 0
    for lo in range(0, H, 256):
        hh = hf[lo:lo + 256]
        m = len(hh)
        s = orient_signs(np.repeat(P[hh[:, 0]], n, axis=0), np.repeat(P[hh[:, 1]], n, axis=0), np.repeat(P[hh[:, 2]], n, axis=0), np.tile(P, (m, 1)))
        front += int((s > 0).sum())
    if front:
        bad.append("%d (hull facet, point) pairs with the point in front" % front)
    return bad


OUTWARD_FACET = ((1, 2, 3), (0, 3, 2), (0, 1, 3), (0, 2, 1))   # the facet opposite slot s with the cell's own vertex s on its negative side


def tables(points, tets):
    """(tetrahedra, neighbors, hull_facets) in the layout of ops.delaunay for ANY cell list (a host triangulator's, say): cells turned
    positive where they are negative, made canonical, then matched facet by facet and hull edge by hull edge.  ValueError when a facet has
    more than two cells or a hull edge does not have exactly two facets."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.array(tets, dtype=np.int64).reshape(-1, 4)
    neg = orient_signs(P[t[:, 0]], P[t[:, 1]], P[t[:, 2]], P[t[:, 3]]) < 0
    t[neg] = t[neg][:, [0, 1, 3, 2]]
    t = canonical(t)
    T = len(t)
    by_facet = {}
    for c in range(T):
        for k in range(4):
            by_facet.setdefault(tuple(sorted(t[c, list(FACET_OF_SLOT[k])])), []).append((c, k))
    nb = np.full((T, 4), -1, dtype=np.int64)
    hull = []
    for key, cells in by_facet.items():
        if len(cells) > 2:
            raise ValueError("facet %s has %d cells" % (key, len(cells)))
        if len(cells) == 2:
            (c0, k0), (c1, k1) = cells
            nb[c0, k0], nb[c1, k1] = c1, c0
        else:
            hull.append(cells[0])
    hull.sort()
    H = len(hull)
    hf = np.array([t[c, list(OUTWARD_FACET[k])] for c, k in hull], dtype=np.int64).reshape(-1, 3)
    inf = np.full((H, 4), -1, dtype=np.int64)
    by_edge = {}
    for h, (c, k) in enumerate(hull):
        nb[c, k] = T + h
        inf[h, 0] = c
        for j in range(3):
            by_edge.setdefault(tuple(sorted(set(hf[h]) - {hf[h, j]})), []).append((h, j))
    for key, sides in by_edge.items():
        if len(sides) != 2:
            raise ValueError("hull edge %s has %d facets" % (key, len(sides)))
        (h0, j0), (h1, j1) = sides
        inf[h0, j0 + 1], inf[h1, j1 + 1] = T + h1, T + h0
    return t, np.concatenate([nb, inf]), hf


def flip23(t, nb):
    """one 2-3 flip: two cells that share a facet become three around the edge of their two apexes (any such pair will do)"""
    T = len(t)
    for c in range(T):
        for k in range(4):
            m = nb[c, k]
            if m >= T or m < c:
                continue
            f = [v for v in t[c] if v != t[c, k]]
            q = [v for v in t[m] if v not in f][0]
            p = t[c, k]
            new = [[p, q, f[0], f[1]], [p, q, f[1], f[2]], [p, q, f[2], f[0]]]
            return np.concatenate([np.delete(t, [c, m], axis=0), np.array(new)])
    raise AssertionError("no interior facet")


# ---- the point sets of the tests --------------------------------------------------------------------------------------------------------
def uniform_points(n, seed=5):
    return np.random.default_rng(seed).random((n, 3))


def cube_face_points(n, seed=6):
    """n points on the six faces of the unit cube plus its eight corners: coplanar hull facets, coplanar quadruples"""
    rng = np.random.default_rng(seed)
    p = rng.random((n - 8, 3))
    face = np.arange(n - 8) % 6
    p[np.arange(n - 8), face // 2] = (face % 2).astype(np.float64)
    corners = np.array([[i, j, k] for i in (0.0, 1.0) for j in (0.0, 1.0) for k in (0.0, 1.0)])
    return np.concatenate([p, corners])


def grid_points(m):
    return np.array([[i, j, k] for i in range(m) for j in range(m) for k in range(m)], dtype=np.float64)


def norm3_points():
    """the 30 integer points of norm 3, all exactly on one sphere: the permutations and signs of (1, 2, 2) and (3, 0, 0)"""
    pts = {p for base in ((1, 2, 2), (3, 0, 0)) for q in itertools.permutations(base) for p in itertools.product(*[(x, -x) for x in q])}
    return np.array(sorted(pts), dtype=np.float64)


def sphere_integer_points(n, radius=171):
    """the first n (lexicographic) integer points of norm exactly `radius`: radius 171 has 2142"""
    r = np.arange(-radius, radius + 1)
    x, y = np.meshgrid(r, r, indexing="ij")
    z2 = radius * radius - x * x - y * y
    z = np.sqrt(np.maximum(z2, 0)).round().astype(np.int64)
    ok = (z2 >= 0) & (z * z == z2)
    pts = {(int(a), int(b), int(s * c)) for a, b, c in zip(x[ok], y[ok], z[ok]) for s in (1, -1)}
    pts = np.array(sorted(pts), dtype=np.float64)
    assert len(pts) >= n
    return pts[:n]
