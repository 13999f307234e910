"""CPU model of the facet-ray walk (the contract of dgnn_ray_walk in include/dgnn_hip.h): plain Python floats (IEEE fp64, every
operation rounding on its own) for the distances, the fp64 filter of csrc/exact_orient.h followed by `fractions.Fraction` for every sign.
No schedule: one ray after the other, the fold in ascending (ray, step) order.

* ray_walk: the rule -- the perturbed side test, the start cells, the steps, the ends, the records and their aggregates;
* crossed_cells: an all-pairs definition that walks nothing: cell t is crossed by ray r when the open segment (p, s) -- or, behind p, the
  open ray away from s -- meets t's open interior, decided with Fractions;
* kuhn_grid: every cube of a lattice split into six tets around its main diagonal, no flat cell: rays along edges, through vertices and in
  facets wherever a sensor is a lattice point;
* finite_neighbors: the [T, 4] table of delaunay_model.tables with -1 for the infinite side.
"""
from __future__ import annotations

import functools
import itertools
import math
from fractions import Fraction

import numpy as np

import delaunay_model as dm

OUTSIDE, INSIDE = 0, 1
SIDES = ("outside", "inside")
STATUS = ("none", "sensor", "hull", "depth", "stuck", "capped")
NONE, SENSOR, HULL, DEPTH, STUCK, CAPPED = range(6)
STATS = ("used", "skipped", "perturbed", "exact_used", "degenerate") + STATUS + ("records", "longest")
OTHERS = ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))
RECORD_KEYS = ("ray", "side", "step", "cell", "slot", "first", "second")


# ---- the exact orientation sign, with the device's filter ---------------------------------------------------------------------------
def _exact(a, b, c, p):
    r = [[Fraction(x[i]) - Fraction(a[i]) for i in range(3)] for x in (b, c, p)]
    d = (r[0][0] * (r[1][1] * r[2][2] - r[1][2] * r[2][1]) - r[0][1] * (r[1][0] * r[2][2] - r[1][2] * r[2][0])
         + r[0][2] * (r[1][0] * r[2][1] - r[1][1] * r[2][0]))
    return (d > 0) - (d < 0)


def orient(a, b, c, p):
    """sign of det[b - a, c - a, p - a] on tuples of floats -> (sign, 1 when the exact stage decided): csrc/exact_orient.h, scalar"""
    ux, uy, uz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    vx, vy, vz = c[0] - a[0], c[1] - a[1], c[2] - a[2]
    wx, wy, wz = p[0] - a[0], p[1] - a[1], p[2] - a[2]
    m0, m1, m2, m3, m4, m5 = vy * wz, vz * wy, vx * wz, vz * wx, vx * wy, vy * wx
    det = ux * (m0 - m1) - uy * (m2 - m3) + uz * (m4 - m5)
    perm = abs(ux) * (abs(m0) + abs(m1)) + abs(uy) * (abs(m2) + abs(m3)) + abs(uz) * (abs(m4) + abs(m5))
    bound = (7.0 + 56.0 * 2.0 ** -53) * 2.0 ** -53 * perm + 2.0 ** -700
    if det > bound:
        return 1, 0
    if -det > bound:
        return -1, 0
    return _exact(a, b, c, p), 1


def axis_up(x):
    """a representable coordinate above x: 0 for a negative one, 1 for 0, 2 x for a positive one"""
    return 0.0 if x < 0.0 else (1.0 if x == 0.0 else 2.0 * x)


class _Ray:
    """the side test of one ray: sigma(u, v) = sign det[s' - p, u - p, v - p], s' = s + (eps, eps^2, eps^3)"""

    def __init__(self, p, s):
        self.p, self.s = p, s
        self.moved = [tuple(axis_up(p[i]) if i == a else p[i] for i in range(3)) for a in range(3)]
        self.exact = 0
        self.perturbed = False

    def orient(self, a, b, c, d):
        g, ex = orient(a, b, c, d)
        self.exact += ex
        return g

    def sigma(self, u, v):
        g = self.orient(self.p, self.s, u, v)
        if g:
            return g
        self.perturbed = True
        for a in range(3):          # det[e_a, u - p, v - p] through p moved up its axis a
            g = self.orient(self.p, self.moved[a], u, v)
            if g:
                return g
        return 0


def crossing(x, y, z):
    """the common sign of three edge signs, 0 when the facet is not crossed"""
    if x >= 0 and y >= 0 and z >= 0 and (x or y or z):
        return 1
    if x <= 0 and y <= 0 and z <= 0 and (x or y or z):
        return -1
    return 0


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _distance(p, d, q0, q1, q2):
    """n . (q0 - p) / (n . d), n = (q1 - q0) x (q2 - q0): dgnn_vertex_rays' dist.  None: a zero denominator or a non-finite value"""
    n = _cross(_sub(q1, q0), _sub(q2, q0))
    den = _dot(n, d)
    if den == 0.0:
        return None
    t = _dot(n, _sub(q0, p)) / den
    return t if math.isfinite(t) else None


def first_rays(ray_vertex, n_vertices):
    rv = np.asarray(ray_vertex, np.int64)
    first = np.full(n_vertices, len(rv), dtype=np.int64)
    np.minimum.at(first, rv, np.arange(len(rv)))
    return first[rv] == np.arange(len(rv))


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def ray_walk(vertices, tetrahedra, neighbors, ray_vertex, sensors, unique=True, outside_depth=0, inside_depth=1):
    """-> dict: "records": dict of RECORD_KEYS -> array, in ascending (ray, side, step); per side s in SIDES "<s>_cell_count" int32 [T],
    "<s>_cell_{first,second}_{min,max,sum}" fp64 [T], "<s>_slot_count" int32 [T, 4], "<s>_slot_{min,max,sum}" fp64 [T, 4]; "ray_status",
    "ray_cells", "ray_start" (the start tet, -1 = none), "ray_starts" (how many tets qualified as the start) int32 [R, 2]; "stats"."""
    V = [tuple(float(x) for x in row) for row in np.asarray(vertices, np.float64).reshape(-1, 3)]
    tets = np.asarray(tetrahedra, np.int64).reshape(-1, 4).tolist()
    nbr = np.asarray(neighbors, np.int64).reshape(-1, 4).tolist()
    rv = np.asarray(ray_vertex, np.int64).reshape(-1)
    S = [tuple(float(x) for x in row) for row in np.asarray(sensors, np.float64).reshape(-1, 3)]
    n_r, n_t = len(rv), len(tets)
    incident = [[] for _ in V]
    for t, row in enumerate(tets):
        for k, a in enumerate(row):
            incident[a].append((t, k))
    is_first = first_rays(rv, len(V)) if unique else np.ones(n_r, dtype=bool)
    depth = (int(outside_depth), int(inside_depth))

    status = np.zeros((n_r, 2), dtype=np.int32)
    cells = np.zeros((n_r, 2), dtype=np.int32)
    start = np.full((n_r, 2), -1, dtype=np.int32)
    starts = np.zeros((n_r, 2), dtype=np.int32)
    rec = {k: [] for k in RECORD_KEYS}
    stats = dict.fromkeys(STATS, 0)

    for r in range(n_r):
        p, s = V[rv[r]], S[r]
        if s == p or not is_first[r]:
            stats["skipped"] += 1
            continue
        stats["used"] += 1
        ray = _Ray(p, s)
        # the start cells: the tets incident to p whose facet opposite p is crossed, forwards with the sign of the tet, backwards against it
        best = [None, None]
        for t, k in incident[rv[r]]:
            q = [V[tets[t][j]] for j in OTHERS[k]]
            D = ray.orient(p, q[0], q[1], q[2])
            sg = (ray.sigma(q[0], q[1]), ray.sigma(q[1], q[2]), ray.sigma(q[2], q[0]))
            c = crossing(*sg)
            if D == 0 or c == 0:
                continue
            side = OUTSIDE if c == D else INSIDE
            starts[r, side] += 1
            if best[side] is None or t < best[side][0]:
                best[side] = (t, k, sg)
        e = _sub(s, p)
        length = math.sqrt(_dot(e, e))
        for side in (OUTSIDE, INSIDE):
            if best[side] is None:
                continue
            d = (e[0] / length, e[1] / length, e[2] / length)
            if side == INSIDE:
                d = (-d[0], -d[1], -d[2])
            c, k, sg = best[side]
            start[r, side] = c
            f = [tets[c][j] for j in OTHERS[k]]
            prev, first, n_cells, steps, recorded = 0.0, 0.0, 0, 0, False          # recorded: the current cell is not the start cell
            while True:
                if side == OUTSIDE and ray.orient(V[f[0]], V[f[1]], V[f[2]], s) != crossing(*sg):          # s is not strictly beyond the exit facet
                    if recorded:
                        _record(rec, r, side, n_cells, c, -1, first, length)
                        n_cells += 1
                    status[r, side] = SENSOR
                    break
                q = [V[tets[c][j]] for j in OTHERS[k]]
                dist = _distance(p, d, q[0], q[1], q[2])
                if dist is None:
                    dist = prev
                    stats["degenerate"] += 1
                prev = dist
                if recorded:
                    _record(rec, r, side, n_cells, c, k, first, dist)
                    n_cells += 1
                    if depth[side] and n_cells == depth[side]:
                        status[r, side] = DEPTH
                        break
                nxt = nbr[c][k]
                if nxt < 0:
                    status[r, side] = HULL
                    break
                steps += 1
                if steps > n_t:
                    status[r, side] = CAPPED
                    break
                row = tets[nxt]
                apex = [j for j in range(4) if row[j] not in f]
                assert len(apex) == 1, "neighbors: cell %d does not hold the facet %s of cell %d" % (nxt, f, c)
                w = row[apex[0]]
                a = [ray.sigma(V[w], V[f[m]]) for m in range(3)]
                cand = [(a[(m + 1) % 3], sg[(m + 1) % 3], -a[(m + 2) % 3]) for m in range(3)]          # the facet opposite f[m]: (w, f[m+1], f[m+2])
                hit = [m for m in range(3) if crossing(*cand[m])]
                if len(hit) != 1:
                    status[r, side] = STUCK
                    break
                m = hit[0]
                c, k, first, recorded = nxt, row.index(f[m]), dist, True
                f, sg = [w, f[(m + 1) % 3], f[(m + 2) % 3]], cand[m]
            cells[r, side] = n_cells
        stats["exact_used"] += ray.exact
        stats["perturbed"] += int(ray.perturbed)

    records = {k: np.array(rec[k], dtype=np.float64 if k in ("first", "second") else np.int32) for k in RECORD_KEYS}
    out = dict(records=records, ray_status=status, ray_cells=cells, ray_start=start, ray_starts=starts)
    out.update(fold(records, n_t))
    for i, name in enumerate(STATUS):
        stats[name] = int((status == i).sum())
    stats["records"] = len(records["ray"])
    stats["longest"] = int(cells.max()) if n_r else 0
    out["stats"] = stats
    return out


def _record(rec, r, side, step, cell, slot, first, second):
    for k, x in zip(RECORD_KEYS, (r, side, step, cell, slot, first, second)):
        rec[k].append(x)


def fold(records, n_t):
    """the aggregates of a record stream, folded in its order (ascending (ray, step) per side): counts, min / max, the sums from 0.0"""
    out = {}
    for side, name in enumerate(SIDES):
        agg = {"cell_first": _Agg((n_t,)), "cell_second": _Agg((n_t,)), "slot": _Agg((n_t, 4))}
        for i in np.nonzero(records["side"] == side)[0]:
            c, k = int(records["cell"][i]), int(records["slot"][i])
            agg["cell_first"].add(c, float(records["first"][i]))
            agg["cell_second"].add(c, float(records["second"][i]))
            if k >= 0:
                agg["slot"].add((c, k), float(records["second"][i]))
        out[name + "_cell_count"] = agg["cell_first"].n
        out[name + "_slot_count"] = agg["slot"].n
        for key, a in agg.items():
            out["%s_%s_min" % (name, key)], out["%s_%s_max" % (name, key)], out["%s_%s_sum" % (name, key)] = a.lo, a.hi, a.sum
    return out


class _Agg:
    def __init__(self, shape):
        self.n = np.zeros(shape, dtype=np.int32)
        self.lo, self.hi, self.sum = np.zeros(shape), np.zeros(shape), np.zeros(shape)

    def add(self, i, d):
        self.lo[i] = d if self.n[i] == 0 else min(self.lo[i], d)
        self.hi[i] = d if self.n[i] == 0 else max(self.hi[i], d)
        self.sum[i] = self.sum[i] + d
        self.n[i] += 1


def walked_cells(out, r, side):
    """the cells ray r touches on a side: its start cell, then the recorded ones"""
    rec = out["records"]
    sel = (rec["ray"] == r) & (rec["side"] == side)
    return ([int(out["ray_start"][r, side])] if out["ray_start"][r, side] >= 0 else []) + rec["cell"][sel].tolist()


# ---- the all-pairs definition --------------------------------------------------------------------------------------------------------
def _integers(*arrays):
    """the fp64 values of the arrays as Python integers on one common power-of-two scale (every double is a dyadic rational)"""
    fr = [[[Fraction(float(x)) for x in row] for row in np.asarray(a, np.float64).reshape(-1, 3)] for a in arrays]
    scale = max([x.denominator for a in fr for row in a for x in row] + [1])
    return [[[int(x * scale) for x in row] for row in a] for a in fr]


def crossed_cells(vertices, tetrahedra, p, s, side):
    """the set of tets whose open interior meets the open segment (p, s) (side 0) or the open ray from p away from s (side 1).  A point
    p + t (s - p) lies inside when all four facet functions f_k(t) = f_k(0) + t g_k are positive (each signed towards the tet's own
    vertex k); exact: integers, the parameters t compared as fractions by cross-multiplication."""
    V = np.asarray(vertices, np.float64)
    tets = np.asarray(tetrahedra, np.int64)
    # a float pre-filter that only ever drops tets far from the ray: the distance of the centroid to the line against the tet's radius
    cen = V[tets].mean(axis=1)
    rad = np.linalg.norm(V[tets] - cen[:, None, :], axis=2).max(axis=1)
    e = np.asarray(s, np.float64) - np.asarray(p, np.float64)
    w = cen - np.asarray(p, np.float64)
    tc = w @ e / (e @ e)
    off = np.linalg.norm(w - np.outer(tc, e), axis=1)
    slack = (1.01 * rad + 1e-9) / np.sqrt(e @ e)
    near = np.nonzero((off <= 1.01 * rad + 1e-9) & (tc <= (1.0 if side == OUTSIDE else 0.0) + slack) & ((tc >= -slack) | (side == INSIDE)))[0]
    ids = np.unique(tets[near])
    ints = _integers(V[ids], [p], [s])
    Q = dict(zip(ids.tolist(), ints[0]))
    P, S = ints[1][0], ints[2][0]
    E = [x - y for x, y in zip(S, P)]
    less = lambda a, b: a[0] * b[1] < b[0] * a[1]          # fractions (numerator, positive denominator)
    out = set()
    for t in near:
        q = [Q[i] for i in tets[t].tolist()]
        lo, hi = ((0, 1), (1, 1)) if side == OUTSIDE else (None, (0, 1))
        ok = True
        for k in range(4):
            q0, q1, q2 = (q[j] for j in OTHERS[k])
            a, b = [x - y for x, y in zip(q1, q0)], [x - y for x, y in zip(q2, q0)]
            n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
            own = sum(x * (y - z) for x, y, z in zip(n, q[k], q0))
            if own == 0:          # a flat tet has no interior
                ok = False
                break
            sgn = 1 if own > 0 else -1
            f0 = sgn * sum(x * (y - z) for x, y, z in zip(n, P, q0))
            g = sgn * sum(x * y for x, y in zip(n, E))
            if g == 0:
                ok = f0 > 0
            elif g > 0:          # inside for t > -f0 / g
                if lo is None or less(lo, (-f0, g)):
                    lo = (-f0, g)
            elif less((f0, -g), hi):          # inside for t < f0 / -g
                hi = (f0, -g)
            if not ok or (lo is not None and not less(lo, hi)):
                ok = False
                break
        if ok:
            out.add(int(t))
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def finite_neighbors(points, tets):
    """(tetrahedra [T, 4], neighbors [T, 4] with -1 for the infinite side) of any cell list, through delaunay_model.tables"""
    t, nb, _ = dm.tables(points, tets)
    nb = nb[:len(t)].copy()
    nb[nb >= len(t)] = -1
    return t.astype(np.int32), nb.astype(np.int32)


def kuhn_grid(m):
    """(points [m^3, 3], tetrahedra, neighbors): the lattice {0..m-1}^3, each of its (m-1)^3 cubes split into the six tets
    (o, o + e_a, o + e_a + e_b, o + (1, 1, 1)) over the orders (a, b, c) of the axes.  The split is the same in every cube, so the tets of
    neighbouring cubes meet in whole facets; no tet is flat."""
    pts = dm.grid_points(m)
    idx = lambda x: (x[0] * m + x[1]) * m + x[2]
    tets = []
    for o in itertools.product(range(m - 1), repeat=3):
        for perm in itertools.permutations(range(3)):
            x, row = list(o), [idx(o)]
            for a in perm:
                x[a] += 1
                row.append(idx(x))
            tets.append(row)
    t, nb = finite_neighbors(pts, tets)
    return pts, t, nb


def general_points(n=150, seed=11, span=1 << 16):
    """n distinct random integer points (as fp64): with integers of 16 bits every determinant of the walk is exact in fp64 as well"""
    rng = np.random.default_rng(seed)
    pts = np.unique(rng.integers(0, span, (2 * n, 3)), axis=0)
    return rng.permutation(pts)[:n].astype(np.float64)


def scipy_cells(points):
    from scipy.spatial import Delaunay
    return finite_neighbors(points, Delaunay(np.asarray(points, np.float64)).simplices)


# ---- the cases of the tests (each computed once, read only) -----------------------------------------------------------------------------

ONE_TET = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
TWO_TETS = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1]])          # the shared facet (0, 1, 2) lies in the plane z = 0
COUNTS = (0, 1, 63, 64, 65, 4097)
CASES = ("general", "general_scaled", "kuhn3", "kuhn4", "kuhn5", "one_tet", "two_tets") + tuple("count_%d" % n for n in COUNTS)


def general_sensors(n, seed=3, span=1 << 16):
    """even rays look at a point of the points' box, odd ones at a point far outside it"""
    rng = np.random.default_rng(seed)
    near, far = rng.integers(0, span, (n, 3)), span // 2 + rng.integers(-4 * span, 4 * span, (n, 3))
    return np.where((np.arange(n) % 2 == 0)[:, None], near, far).astype(np.float64)


def kuhn_sensors(m, seed):
    """two rays per lattice point: to another lattice point (along edges, through vertices, in facets), and to a random integer point of a
    box two units wider (the same, and past the hull)"""
    rng = np.random.default_rng(seed)
    n = m ** 3
    rv = np.concatenate([np.arange(n), np.arange(n)])
    return rv, np.concatenate([rng.integers(0, m, (n, 3)), rng.integers(-2, m + 2, (n, 3))]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(which):
    """-> (vertices, tetrahedra, neighbors, ray_vertex, sensors, keyword arguments of ray_walk, the model's result)"""
    kw = dict(unique=True, outside_depth=0, inside_depth=0)
    if which.startswith("general"):
        v = general_points()
        tets, nbr = scipy_cells(v)
        rv, s = np.arange(len(v)), general_sensors(len(v))
        if which == "general_scaled":          # every coordinate 2^20 + k 2^-20: exact in fp64, differences far below the magnitudes
            v, s = v * 2.0 ** -20 + 2.0 ** 20, s * 2.0 ** -20 + 2.0 ** 20
    elif which.startswith("kuhn"):
        m = int(which[4:])
        v, tets, nbr = kuhn_grid(m)
        rv, s = kuhn_sensors(m, seed=m)
        kw["unique"] = False
    elif which == "one_tet":
        v = ONE_TET
        tets, nbr = finite_neighbors(v, [[0, 1, 2, 3]])
        rv = np.array([0, 3, 3, 1, 2])          # a far sensor; one inside the cell; one exactly on its facet; along an edge; s == p
        s = np.array([[5.0, 5, 5], [0.25, 0.25, 0.25], [0.25, 0.25, 0], [-1, 2, 0], [0, 1, 0]])
        kw["unique"] = False
    elif which == "two_tets":
        v = TWO_TETS
        tets, nbr = finite_neighbors(v, [[0, 2, 1, 4], [0, 1, 2, 3]])
        # from vertex 3 down through the shared facet's interior, through its edge (1, 2), along the edges 3-0-4 through vertex 0, through
        # vertex 1; from vertex 4 up to a sensor inside the other cell and to one exactly on the shared facet
        rv = np.array([3, 3, 3, 3, 4, 4])
        s = np.array([[0.25, 0.25, -2], [1, 1, -1], [0, 0, -0.5], [2, 0, -1], [0.25, 0.25, 0.5], [0.25, 0.25, 0]], dtype=np.float64)
        kw["unique"] = False
    else:          # many rays onto the few vertices of the 3^3 grid, half of them onto its centre: long runs per cell in the fold
        n = int(which[6:])
        v, tets, nbr = kuhn_grid(3)
        rng = np.random.default_rng(n)
        rv = np.where(np.arange(n) % 2 == 1, 13, np.arange(n) % len(v))
        s = rng.integers(-128, 256, (n, 3)) / 64.0          # off the lattice: few ties, the long run is what this case is for
        kw["unique"] = False
    want = ray_walk(v, tets, nbr, rv, s, **kw)
    for a in (v, tets, nbr, rv, s):
        a.setflags(write=False)
    return v, tets, nbr, rv, s, kw, want
