"""The two subsampling rules of include/dgnn_hip.h restated in numpy over all pairs, operation for operation: `voxel_subsample`
(floor cells, numbering by first member, the centroid in fixed_sum.h's order, the nearest member) and `min_distance_thin` (the sequential greedy
in the order of (key, index), its dependency depth, the splitmix64 key), with the independent checks the tests hold a result to.  No GPU, no torch;
the clouds are knn_model's."""
import numpy as np

from knn_model import FIXED_SUM_CHUNK, d2_matrix

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
VOXEL_LIMIT = 2.0 ** 20


def mix(z):
    """the splitmix64 finaliser, modulo 2^64"""
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def thin_key(seed, i):
    return mix(mix(seed + GOLDEN) + i)


# ---- voxel grid ------------------------------------------------------------------------------------------------------------------------
def serial_chunk_sum(x):
    """fixed_sum.h: s = 0, s += x over a chunk of 256; total = 0, total += s over the chunks"""
    total = 0.0
    for t in range(0, len(x), FIXED_SUM_CHUNK):
        total = total + float(np.cumsum(np.concatenate([[0.0], x[t:t + FIXED_SUM_CHUNK]]))[-1])
    return total


def voxel_subsample(points, h, origin=(0.0, 0.0, 0.0)):
    """-> dict of voxel int32 [n], count, first, nearest int32 [m], centroid fp64 [m, 3], m"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    h = float(h)
    if not (np.isfinite(h) and h > 0):
        raise ValueError("the voxel size is not a finite positive number")
    if not np.isfinite(p).all():
        raise ValueError("a non-finite coordinate")
    c = np.floor((p - np.asarray(origin, dtype=np.float64)) / h)
    if not (np.abs(c) < VOXEL_LIMIT).all():
        raise ValueError("a voxel coordinate outside (-2^20, 2^20)")
    rows, voxel = {}, np.zeros(len(p), np.int32)
    for i, key in enumerate(map(tuple, c.astype(np.int64))):          # ascending index: a voxel's number is that of its first member
        voxel[i] = rows.setdefault(key, len(rows))
    m = len(rows)
    count, first, nearest, centroid = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, 3))
    for v in range(m):
        members = np.flatnonzero(voxel == v)
        count[v], first[v] = len(members), members[0]
        centroid[v] = [serial_chunk_sum(p[members, a]) / float(len(members)) for a in range(3)]
        d2 = d2_matrix(centroid[v], p[members])[0]
        nearest[v] = members[np.argmin(d2)]          # the first of the smallest: the lowest index
    return dict(voxel=voxel, count=count, first=first, nearest=nearest, centroid=centroid, m=m)


# ---- thinning --------------------------------------------------------------------------------------------------------------------------
def thin_order(n, priority=None, seed=0):
    """the points in the order of (key_i, i)"""
    if priority is not None:
        keys = [int(x) for x in np.asarray(priority, dtype=np.int64).reshape(-1)]
        assert len(keys) == n
    else:
        keys = [thin_key(seed, i) for i in range(n)]
    return sorted(range(n), key=lambda i: (keys[i], i))


def conflicts(points, radius):
    """bool [n, n]: d2(i, j) < fl(r r), the diagonal off"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    r = np.float64(radius)
    c = d2_matrix(p, p) < r * r
    np.fill_diagonal(c, False)
    return c


def min_distance_thin(points, radius, priority=None, seed=0):
    """-> (keep bool [n], depth): the sequential greedy, and the number of rounds the parallel form needs when every round sees only the states
    of the round before (a point is decided one round after its first kept earlier conflict, or after the last of them when none is kept);
    reading states in place can only be quicker"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if not (np.isfinite(radius) and radius >= 0):
        raise ValueError("the radius is not a finite number >= 0")
    n = len(p)
    c = conflicts(p, radius)
    keep, decided_in, seen = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, bool)
    for i in thin_order(n, priority, seed):
        earlier = np.flatnonzero(c[i] & seen)
        kept = earlier[keep[earlier]]
        keep[i] = len(kept) == 0
        decided_in[i] = 1 + (decided_in[kept].min() if len(kept) else (decided_in[earlier].max() if len(earlier) else 0))
        seen[i] = True
    return keep, int(decided_in.max()) if n else 0


def check_thinning(points, radius, keep, priority=None, seed=0):
    """the two properties that make `keep` the greedy answer's kind, from `keep` alone: (a) no two kept points conflict; (b) every removed
    point has a kept conflict earlier in the order.  -> (a, b)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    keep = np.asarray(keep, dtype=bool)
    n = len(p)
    c = conflicts(p, radius)
    rank = np.zeros(n, np.int64)
    rank[thin_order(n, priority, seed)] = np.arange(n)
    a = not c[np.ix_(keep, keep)].any()
    earlier_kept = c & keep[None, :] & (rank[None, :] < rank[:, None])
    b = bool(earlier_kept[~keep].any(axis=1).all())
    return a, b
