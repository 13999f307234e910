"""CPU model of the manifold repair (the contract of dgnn_vertex_components / dgnn_manifold_repair).  It does not share the
device's formulation: where the device joins the 4 T corners in one union-find and reads the components off its roots, the model keeps
an explicit list of the cells around every vertex and runs a breadth-first search over them, with one extra node for the infinite cell.

* `vertex_components`: a(v), b(v) and the components themselves (sets of cells) from that search;
* `repair`: the rounds of the rule exactly as DESIGN §31 words it -- candidates, the (cost, smallest cell) order, the claims, the winners,
  the mark -- with the state after every round kept, and a switch that leaves the mark out (to show why it is there);
* `face_check`: the criterion's yardstick, which is NOT the criterion restated: the interface triangles are extracted, the faces on every
  undirected edge counted and the fans around every vertex found by joining the face corners that share a link edge.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np

INF = -1          # the node of the infinite cell in a star
STAT_KEYS = ("rounds", "moves", "flipped_cells", "to_inside", "to_outside", "flipped_cost", "singular_before", "singular_after")
_OTHERS = ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))


def scipy_scene(points):
    """-> (tetrahedra int32 [T, 4], neighbors int32 [T, 4]) of scipy's Delaunay; slot k = the cell across the facet opposite vertex k"""
    from scipy.spatial import Delaunay

    tri = Delaunay(np.asarray(points, dtype=np.float64))
    return tri.simplices.astype(np.int32), tri.neighbors.astype(np.int32)


def stars(tets, n_vertices):
    """star[v] = the (cell, slot) pairs with tets[cell][slot] == v, in ascending cell order"""
    out = [[] for _ in range(n_vertices)]
    for c, row in enumerate(np.asarray(tets).tolist()):
        for k, v in enumerate(row):
            out[v].append((c, k))
    return out


def star_components(star, nbr, labels):
    """The components of one vertex's star graph -> list of (side, frozenset of cells, has_inf), a lone infinite node included (as
    (1, frozenset(), True)).  Two star cells are joined when they share a facet through the vertex and carry the same label; an outside
    cell with the infinite cell behind such a facet is joined to INF."""
    cells = {c: k for c, k in star}
    has_inf = any(nbr[c][j] < 0 for c, k in star for j in _OTHERS[k])
    adj = defaultdict(list)
    for c, k in star:
        for j in _OTHERS[k]:
            n = nbr[c][j]
            if n < 0:
                if labels[c] == 1:
                    adj[c].append(INF)
                    adj[INF].append(c)
            elif n in cells and labels[n] == labels[c]:
                adj[c].append(n)
    seen, comps = set(), []
    for start in list(cells) + ([INF] if has_inf else []):
        if start in seen:
            continue
        seen.add(start)
        queue, members = [start], []
        while queue:
            x = queue.pop()
            members.append(x)
            for y in adj[x]:
                if y not in seen:
                    seen.add(y)
                    queue.append(y)
        side = 1 if INF in members else int(labels[members[0]])
        comps.append((side, frozenset(m for m in members if m != INF), INF in members))
    return comps


def vertex_components(tets, nbr, labels, n_vertices):
    """-> (a int32 [V], b int32 [V], number of singular vertices)"""
    nbr, labels = np.asarray(nbr).tolist(), np.asarray(labels).tolist()
    a, b = np.zeros(n_vertices, dtype=np.int32), np.zeros(n_vertices, dtype=np.int32)
    for v, star in enumerate(stars(tets, n_vertices)):
        for side, _, _ in star_components(star, nbr, labels):
            (a if side == 0 else b)[v] += 1
    return a, b, int(((a > 1) | (b > 1)).sum())


def repair(tets, nbr, labels, n_vertices, cost=None, max_rounds=None, mark=True):
    """The rounds of DESIGN §31 -> (labels int32 [T], stats dict of STAT_KEYS, flipped int32 [T], history): history[r] = the labels after
    r + 1 rounds.  mark=False lets a cell flip again (the rule without its termination argument; bound it with max_rounds)."""
    tets = np.asarray(tets)
    T = len(tets)
    nbr = np.asarray(nbr).tolist()
    lab = [int(x) for x in np.asarray(labels)]
    cost = [1] * T if cost is None else [int(x) for x in np.asarray(cost)]
    star = stars(tets, n_vertices)
    flipped = [0] * T
    times = [0] * T
    comps = [None] * n_vertices
    stats = dict.fromkeys(STAT_KEYS, 0)
    history = []

    def singular(v):
        if comps[v] is None:
            comps[v] = star_components(star[v], nbr, lab)
        n = [sum(1 for s, _, _ in comps[v] if s == side) for side in (0, 1)]
        return n, (n[0] > 1 or n[1] > 1)

    while True:
        moves, n_singular = {}, 0
        for v in range(n_vertices):
            n, bad = singular(v)
            if not bad:
                continue
            n_singular += 1
            best = None
            for side, cells, has_inf in comps[v]:
                if n[side] < 2 or has_inf or (mark and any(flipped[c] for c in cells)):
                    continue
                key = (sum(cost[c] for c in cells), min(cells))
                if best is None or key < best[0]:
                    best = (key, cells)
            if best is not None:
                moves[v] = best[1]
        if stats["rounds"] == 0:
            stats["singular_before"] = n_singular
        stats["singular_after"] = n_singular
        if not moves or (max_rounds is not None and stats["rounds"] >= max_rounds):
            break
        claim = {}
        for v in sorted(moves):
            for c, _ in star[v]:
                claim.setdefault(c, v)            # ascending v: the first claim is the lowest
        winners = [v for v in moves if all(claim[c] == v for c, _ in star[v])]
        assert winners and min(moves) in winners
        for v in winners:
            for c in moves[v]:
                stats["to_inside" if lab[c] == 1 else "to_outside"] += 1
                stats["flipped_cost"] += cost[c]
                lab[c] ^= 1
                flipped[c] = 1
                times[c] += 1
                for u in tets[c]:
                    comps[int(u)] = None
        stats["moves"] += len(winners)
        stats["rounds"] += 1
        history.append(np.asarray(lab, dtype=np.int32))
    stats["flipped_cells"] = stats["to_inside"] + stats["to_outside"]
    stats["max_flips_of_a_cell"] = max(times) if T else 0
    return np.asarray(lab, dtype=np.int32), stats, np.asarray(flipped, dtype=np.int32), history


# ---- the yardstick: the interface as a triangle mesh ---------------------------------------------------------------------------------
def interface_faces(tets, nbr, labels):
    """the facets between an inside cell and an outside one (the infinite cell is outside), each once, as vertex triples [K, 3]"""
    tets, nbr, labels = np.asarray(tets), np.asarray(nbr), np.asarray(labels)
    faces = []
    for c in np.nonzero(labels == 0)[0]:
        for k in range(4):
            n = nbr[c, k]
            if n < 0 or labels[n] == 1:
                faces.append([tets[c, j] for j in _OTHERS[k]])
    return np.asarray(faces, dtype=np.int64).reshape(-1, 3)


def face_check(tets, nbr, labels):
    """-> dict(boundary_edges, nonmanifold_edges, multi_fan_vertices) of the interface mesh: faces per undirected edge (1 = boundary,
    3 or more = non-manifold), and the vertices whose face corners, joined where two faces share an edge through the vertex, fall into more
    than one fan"""
    faces = interface_faces(tets, nbr, labels).tolist()
    on_edge = defaultdict(int)
    corners = defaultdict(list)            # v -> [(face, the two link vertices)]
    for f, (x, y, z) in enumerate(faces):
        for u, w in ((x, y), (y, z), (z, x)):
            on_edge[(min(u, w), max(u, w))] += 1
        corners[x].append((f, y, z))
        corners[y].append((f, x, z))
        corners[z].append((f, x, y))
    multi = 0
    for v, cs in corners.items():
        group = {f: f for f, _, _ in cs}

        def find(f):
            while group[f] != f:
                f = group[f]
            return f

        first = {}
        for f, p, q in cs:
            for link in (p, q):
                if link in first:
                    ra, rb = find(first[link]), find(f)
                    group[max(ra, rb)] = min(ra, rb)
                else:
                    first[link] = f
        multi += len({find(f) for f in group}) > 1
    counts = list(on_edge.values())
    return dict(boundary_edges=sum(n == 1 for n in counts), nonmanifold_edges=sum(n >= 3 for n in counts), multi_fan_vertices=multi)


def facets_of(tets, nbr):
    """(facets int32 [F, 3], nfacets int32 [F, 2]) in `_3dt.npz` layout: every facet once, from its lower cell (hull facets: -1 second)"""
    tets, nbr = np.asarray(tets), np.asarray(nbr)
    c, k = np.nonzero((nbr < 0) | (nbr > np.arange(len(tets))[:, None]))
    keep = np.ones((len(c), 4), dtype=bool)
    keep[np.arange(len(c)), k] = False
    return tets[c][keep].reshape(-1, 3).astype(np.int32), np.stack([c, nbr[c, k]], axis=1).astype(np.int32)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def uniform_points(n, seed):
    return np.random.default_rng(seed).random((n, 3))


def grid_points(n=5):
    return np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)


def sphere_and_centre_points(n=200, seed=0):
    """n points on the unit sphere and the centre: the centre's star is every cell"""
    d = np.random.default_rng(seed).standard_normal((n, 3))
    return np.concatenate([d / np.linalg.norm(d, axis=1, keepdims=True), np.zeros((1, 3))])


def sphere_labels(points, tets, centre=0.5, radius=0.3, noise=0.0, seed=0):
    """0 where the cell's centroid lies within the sphere, then a fraction `noise` of the cells, drawn with `seed`, inverted"""
    cen = np.asarray(points)[np.asarray(tets)].mean(axis=1)
    lab = (np.linalg.norm(cen - centre, axis=1) > radius).astype(np.int32)
    return lab ^ (np.random.default_rng(seed).random(len(lab)) < noise).astype(np.int32)


def random_labels(n, p_inside, seed):
    return (np.random.default_rng(seed).random(n) >= p_inside).astype(np.int32)


def hull_vertices(tets, nbr):
    tets, nbr = np.asarray(tets), np.asarray(nbr)
    out = set()
    for c, k in zip(*np.nonzero(nbr < 0)):
        out.update(int(tets[c, j]) for j in _OTHERS[k])
    return out


def cell_pairs_sharing(tets, nbr, n_shared):
    """the pairs (c, d), c < d, of cells without a hull vertex that share exactly n_shared vertices, in ascending order"""
    tets = np.asarray(tets)
    hull = hull_vertices(tets, nbr)
    sets = [set(row) for row in tets.tolist()]
    inner = [c for c in range(len(tets)) if not (sets[c] & hull)]
    return [(c, d) for i, c in enumerate(inner) for d in inner[i + 1:] if len(sets[c] & sets[d]) == n_shared]


# ---- the scenes of the tests: name -> points, labels --------------------------------------------------------------------------------------
SCENES = {   # name: (points, labels(points, tets), clean = the repair has to end without a stuck vertex)
    "u60_n30": (lambda: uniform_points(60, 1), lambda p, t: sphere_labels(p, t, noise=0.30, seed=10), True),
    "u300_n0": (lambda: uniform_points(300, 1), lambda p, t: sphere_labels(p, t, noise=0.0, seed=2), True),
    "u300_n2": (lambda: uniform_points(300, 1), lambda p, t: sphere_labels(p, t, noise=0.02, seed=2), True),
    "u300_n5": (lambda: uniform_points(300, 1), lambda p, t: sphere_labels(p, t, noise=0.05, seed=2), True),
    "u800_n0": (lambda: uniform_points(800, 1), lambda p, t: sphere_labels(p, t, noise=0.0, seed=2), True),
    "u800_n2": (lambda: uniform_points(800, 1), lambda p, t: sphere_labels(p, t, noise=0.02, seed=2), True),
    "u800_n5": (lambda: uniform_points(800, 1), lambda p, t: sphere_labels(p, t, noise=0.05, seed=2), True),
    "grid5_n10": (lambda: grid_points(5), lambda p, t: sphere_labels(p, t, centre=2.0, radius=1.6, noise=0.10, seed=3), True),
    "sphere_centre": (lambda: sphere_and_centre_points(200, 0), lambda p, t: random_labels(len(t), 0.5, 4), False),
    "u300_n50": (lambda: uniform_points(300, 1), lambda p, t: sphere_labels(p, t, noise=0.50, seed=5), False),
}


def margin_cost(n, seed=0):
    """a stand-in for the `margin` cost of generate: ints in [0, 2^20] with many ties"""
    return (np.random.default_rng(seed).integers(0, 40, n) ** 4 % (2 ** 20 + 1)).astype(np.int32)


def hand_cases(tets, nbr):
    """Small labellings on one triangulation whose outcome can be reasoned out -> name: dict(labels, cost or None, flips = the cells
    that have to change side, sorted).  Cells are chosen away from the hull unless the case is about the hull."""
    tets, nbr = np.asarray(tets), np.asarray(nbr)
    T = len(tets)
    sets = [set(row) for row in tets.tolist()]

    def only(*inside):
        lab = np.ones(T, dtype=np.int32)
        lab[list(inside)] = 0
        return lab

    def costs(**kw):
        c = np.ones(T, dtype=np.int32)
        for k, x in kw.items():
            c[int(k[1:])] = x
        return c

    out = {}
    c, d = cell_pairs_sharing(tets, nbr, 2)[0]                       # two inside cells that share only an edge: the lower id goes
    out["edge_pair"] = dict(labels=only(c, d), cost=None, flips=[c])
    out["edge_pair_cost"] = dict(labels=only(c, d), cost=costs(**{"c%d" % c: 5}), flips=[d])       # ... unless it costs more
    c, d = cell_pairs_sharing(tets, nbr, 1)[0]                       # ... that share only a vertex
    out["vertex_pair"] = dict(labels=only(c, d), cost=None, flips=[c])
    hull_cell = int(np.nonzero((nbr < 0).sum(axis=1) == 1)[0][0])    # one inside cell with one hull facet: a ball, nothing to repair
    out["hull_inside"] = dict(labels=only(hull_cell), cost=None, flips=[])
    out["all_inside"] = dict(labels=np.zeros(T, dtype=np.int32), cost=None, flips=[])
    out["all_outside"] = dict(labels=np.ones(T, dtype=np.int32), cost=None, flips=[])
    hull = hull_vertices(tets, nbr)
    pocket = next(c for c in range(T) if not (sets[c] & hull))       # a closed outside pocket away from the hull
    lab = np.zeros(T, dtype=np.int32)
    lab[pocket] = 1
    out["pocket"] = dict(labels=lab, cost=None, flips=[])
    # a lone cell c1 and a pair c2 | c3 (sharing a facet) that meet in one vertex only: the pair is the larger component and, with
    # cost[c1] = 10, the cheaper one
    for c1, c2 in cell_pairs_sharing(tets, nbr, 1):
        (v,) = sets[c1] & sets[c2]
        for c3 in nbr[c2]:
            if c3 >= 0 and not (sets[c3] & hull) and sets[c1] & sets[c3] == {v}:
                out["larger_cheaper"] = dict(labels=only(c1, c2, int(c3)), cost=costs(**{"c%d" % c1: 10}), flips=sorted([c2, int(c3)]))
                out["larger_dearer"] = dict(labels=only(c1, c2, int(c3)), cost=None, flips=[c1])
                return out
    raise AssertionError("no lone cell and pair around one vertex in this triangulation")


def canonical_order(points, tets, nbr):
    """The same cells in the form ops.delaunay returns them: every row positively oriented with its smallest vertex first and, among its
    even permutations, the lexicographically smallest; rows sorted lexicographically; the neighbour table carried along."""
    p, tets, nbr = np.asarray(points, dtype=np.float64), np.asarray(tets, dtype=np.int64).copy(), np.asarray(nbr, dtype=np.int64).copy()
    a = p[tets[:, 0]]
    det = np.einsum("ij,ij->i", p[tets[:, 1]] - a, np.cross(p[tets[:, 2]] - a, p[tets[:, 3]] - a))
    neg = det < 0
    tets[neg, 2], tets[neg, 3] = tets[neg, 3].copy(), tets[neg, 2].copy()
    nbr[neg, 2], nbr[neg, 3] = nbr[neg, 3].copy(), nbr[neg, 2].copy()
    perms = np.array(((0, 1, 2, 3), (0, 2, 3, 1), (0, 3, 1, 2), (1, 0, 3, 2), (1, 2, 0, 3), (1, 3, 2, 0), (2, 0, 1, 3), (2, 1, 3, 0), (2, 3, 0, 1),
                      (3, 0, 2, 1), (3, 1, 0, 2), (3, 2, 1, 0)))
    key = tets[:, perms[:, 0]] * (len(p) + 1) + tets[:, perms[:, 1]]
    sel = perms[np.argmin(key, axis=1)]
    tets, nbr = np.take_along_axis(tets, sel, axis=1), np.take_along_axis(nbr, sel, axis=1)
    order = np.lexsort((tets[:, 3], tets[:, 2], tets[:, 1], tets[:, 0]))
    new_id = np.empty(len(tets) + 1, dtype=np.int64)
    new_id[order] = np.arange(len(tets))
    new_id[-1] = -1
    return tets[order].astype(np.int32), new_id[nbr[order]].astype(np.int32)
