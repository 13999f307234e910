"""The sampled k-hop block construction of dgnn_amd.sampler.NeighborSampler (sizes[h] > 0), restated in numpy integer arithmetic and
independent of the library: the model that tests/test_gpu_sampled_blocks.py holds the GPU builder to, exactly.

``sizes[h]`` applies to builder hop ``h`` (hop 0 = the batch's own neighbourhood = the innermost block, LAST in the returned list).  A target
with global id ``g`` and in-degree ``d`` keeps all its in-edges when ``sizes[h] == -1`` or ``d <= sizes[h]``; otherwise the ``k = sizes[h]`` of
them with the smallest keys

    key(seed, draw, h, g, j) = mix(mix(mix(seed + 0x9E3779B97F4A7C15 * (draw + 1)) ^ g) + ((h << 32) | j))      (modulo 2^64)

where ``j = 0..d-1`` ranks the in-edges in plan order (ascending edge position) and ``mix`` is the splitmix64 finaliser; ties go to the smaller
``j``.  Kept edges stay in plan order; targets keep their local positions; new sources are appended in order of first appearance among kept
edges; ``e_id`` is the graph edge id; the list is reversed at the end (outermost block first).
"""
import numpy as np

_U = np.uint64
GOLDEN = _U(0x9E3779B97F4A7C15)


def mix(z):
    """splitmix64 finaliser on uint64 scalars / arrays (wrapping arithmetic)"""
    z = np.asarray(z, dtype=_U)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def keys(seed, draw, hop, g, d):
    """the d keys of target g at hop `hop`, uint64 [d]"""
    with np.errstate(over="ignore"):
        base = mix(_U(int(seed) & (2 ** 64 - 1)) + GOLDEN * _U(int(draw) + 1))
        b = mix(base ^ _U(int(g)))
        return mix(b + ((_U(int(hop)) << _U(32)) | np.arange(d, dtype=_U)))


def kept(seed, draw, hop, g, d, size):
    """ranks j (ascending) of the in-edges that target g keeps"""
    if size == -1 or d <= size:
        return np.arange(d, dtype=np.int64)
    k = keys(seed, draw, hop, g, d)
    order = np.lexsort((np.arange(d), k))       # by key, ties by smaller j
    return np.sort(order[:size]).astype(np.int64)


def plan(edge_index, n_nodes):
    """(rowptr, src, eid) of the by-destination plan: in-edges of a node in ascending edge position"""
    src, dst = np.asarray(edge_index[0], np.int64), np.asarray(edge_index[1], np.int64)
    eid = np.argsort(dst, kind="stable")
    rowptr = np.zeros(n_nodes + 1, dtype=np.int64)
    np.add.at(rowptr, dst + 1, 1)
    return np.cumsum(rowptr), src[eid], eid.astype(np.int64)


def sampled_blocks(edge_index, n_nodes, batch, sizes, seed, draw, with_off=False):
    """-> (n_id int64, [(edge_index_local int64 [2, E_l], e_id int64 [E_l], (n_src, n_dst)), ...]) outermost block first; with_off: every triple
    is followed by the block's row offsets int64 [n_dst + 1]."""
    if any(int(s) == 0 or int(s) < -1 for s in sizes):
        raise ValueError("sizes: -1 or > 0")
    rowptr, psrc, peid = plan(edge_index, n_nodes)
    n_id = np.asarray(batch, dtype=np.int64)
    adjs = []
    for hop, size in enumerate(int(s) for s in sizes):
        n_dst = n_id.shape[0]
        pos = {int(g): i for i, g in enumerate(n_id)}
        new, rows, cols, e_l, off = [], [], [], [], [0]
        for li, g in enumerate(n_id):
            b, e = int(rowptr[g]), int(rowptr[g + 1])
            for j in kept(seed, draw, hop, int(g), e - b, size):
                s = int(psrc[b + j])
                p = pos.get(s)
                if p is None:
                    p = pos[s] = len(pos)
                    new.append(s)
                rows.append(li)
                cols.append(p)
                e_l.append(int(peid[b + j]))
            off.append(len(rows))
        n_id = np.concatenate([n_id, np.asarray(new, dtype=np.int64)])
        blk = (np.asarray([cols, rows], dtype=np.int64).reshape(2, -1), np.asarray(e_l, dtype=np.int64), (int(n_id.shape[0]), n_dst))
        adjs.append(blk + (np.asarray(off, dtype=np.int64),) if with_off else blk)
    return n_id, adjs[::-1]


# ---- the graphs the tests share ------------------------------------------------------------------------------------------------------
def regular_graph():
    """a 4-regular symmetric graph of about 2000 cells in the reference's adjacency layout -> (edge_index int64 [2, 4n], n)"""
    from dgnn_amd.synthetic import delaunay_tet_graph
    adj, _, _ = delaunay_tet_graph(300, seed=5)
    return np.ascontiguousarray(adj.T.astype(np.int64)), adj.shape[0] // 4


def irregular_graph(n=600, seed=9):
    """a directed graph of n nodes with in-degrees spanning 0..12 (every value present), distinct sources per destination, no self loops; the
    edge list is sorted by source, so that a destination's in-edges in edge order have ascending sources (PyG's order = plan order)
    -> (edge_index int64 [2, E], n)"""
    rng = np.random.default_rng(seed)
    deg = np.concatenate([np.arange(13), rng.integers(0, 13, n - 13)])
    rng.shuffle(deg)
    src, dst = [], []
    for v in range(n):
        others = np.delete(np.arange(n), v)
        s = rng.choice(others, size=int(deg[v]), replace=False)
        src.append(s)
        dst.append(np.full(int(deg[v]), v))
    src, dst = np.concatenate(src), np.concatenate(dst)
    order = np.lexsort((dst, src))
    return np.stack([src[order], dst[order]]).astype(np.int64), n
