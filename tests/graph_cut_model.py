"""CPU model of the two-label graph cut of processing/generate_mesh.graph_cut (the contract of dgnn_graph_cut_binary).

* costs: the reference's own expression on its float32 CPU tensor, ``(prediction[:, [1, 0]] * unary_weight).round()`` (fp32 product,
  half to even), as int64; label 0 = inside, 1 = outside;
* Potts weight: ``np.ones(F, int64) * binary_weight`` converted to integers (truncation);
* energy E(l) = sum_i D_i(l_i) + w * #{rows (i, j): l_i != l_j} (duplicate rows add up, self-loops never count);
* the answer: the minimiser with the fewest outside cells (unique -- the outside sets of the minimisers are closed under intersection).

``brute_force`` enumerates every labelling (n <= 14); ``solve`` runs scipy's Dinic maximum flow and takes the nodes that reach t in the
residual graph (the minimal sink side = the canonical labels).
"""
from __future__ import annotations

import numpy as np
import torch


def unary_costs(prediction, unary_weight) -> np.ndarray:
    """int64 [n, 2]: D[:, 0] = cost of inside, D[:, 1] = cost of outside"""
    pred = torch.as_tensor(np.asarray(prediction, dtype=np.float32))[:, [1, 0]]
    return (pred * unary_weight).round().numpy().astype(np.int64)


def potts_weight(binary_weight, n_rows=1) -> int:
    return int((np.ones(max(n_rows, 1), dtype=np.int64) * binary_weight).astype(np.int64)[0])


def energy(labels, D, edges, w) -> int:
    labels = np.asarray(labels).astype(np.int64)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    unary = int(D[np.arange(len(labels)), labels].sum())
    return unary + int(w) * int((labels[edges[:, 0]] != labels[edges[:, 1]]).sum())


def brute_force(prediction, edges, unary_weight, binary_weight):
    """-> (labels int32 [n], energy): every labelling, the least energy, then the fewest outside cells"""
    D = unary_costs(prediction, unary_weight)
    w = potts_weight(binary_weight)
    n = D.shape[0]
    assert n <= 14
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    L = (np.arange(1 << n, dtype=np.int64)[:, None] >> np.arange(n)) & 1          # [2^n, n]
    E = D[np.arange(n), L].sum(1) + w * (L[:, edges[:, 0]] != L[:, edges[:, 1]]).sum(1)
    best = E.min()
    cand = np.nonzero(E == best)[0]
    ones = L[cand].sum(1)
    pick = cand[ones == ones.min()]
    assert len(pick) == 1, "the minimiser with the fewest outside cells is unique"
    return L[pick[0]].astype(np.int32), int(best)


def solve(prediction, edges, unary_weight, binary_weight):
    """-> (labels int32 [n], energy, flow) by scipy.sparse.csgraph.maximum_flow(method='dinic') + a BFS to t over the residual"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import breadth_first_order, maximum_flow

    D = unary_costs(prediction, unary_weight)
    w = potts_weight(binary_weight)
    n = D.shape[0]
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    s, t = n, n + 1
    cs = np.maximum(D[:, 1] - D[:, 0], 0)
    ct = np.maximum(D[:, 0] - D[:, 1], 0)
    e = edges[edges[:, 0] != edges[:, 1]]
    nodes = np.arange(n)
    rows = np.concatenate([np.full(n, s), nodes, e[:, 0], e[:, 1]])
    cols = np.concatenate([nodes, np.full(n, t), e[:, 1], e[:, 0]])
    caps = np.concatenate([cs, ct, np.full(2 * len(e), w, dtype=np.int64)])
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
    E = energy(labels, D, edges, w)
    flow = int(res.flow_value)
    assert E == flow + int(np.minimum(D[:, 0], D[:, 1]).sum()), "max-flow / min-cut identity"
    return labels, E, flow


def interface_faces(labels_finite, nfacets, facets):
    """numpy restatement of the reference's interface loop (generate_mesh.py:93-105): infinite cell (-1) = outside"""
    lab = np.append(np.asarray(labels_finite), 1)
    cells = np.where(nfacets < 0, len(labels_finite), nfacets)
    keep = lab[cells[:, 0]] != lab[cells[:, 1]]
    return facets[keep]


def delaunay_facet_graph(n_points, seed=0):
    """finite-finite facets (each once) of synthetic.delaunay_tet_graph: (edges int32 [F, 2], centroids [n_finite, 3], n_finite)"""
    from dgnn_amd.synthetic import delaunay_tet_graph

    adj, cent, nf = delaunay_tet_graph(n_points, seed=seed)
    a = adj[(adj[:, 0] < nf) & (adj[:, 1] < nf) & (adj[:, 0] < adj[:, 1])]
    return np.ascontiguousarray(a, dtype=np.int32), cent[:nf], nf


def coherent_logits(cent, seed=0, noise=2.0, scale=40.0):
    """a sphere's signed distance at the cell centroids (inside: class 0 larger) plus N(0, noise^2)"""
    rng = np.random.default_rng(seed)
    sd = np.linalg.norm(cent - 0.5, axis=1) - 0.3
    out = np.empty((len(cent), 2), dtype=np.float32)
    out[:, 0] = -scale * sd + rng.normal(0, noise, len(cent))
    out[:, 1] = scale * sd + rng.normal(0, noise, len(cent))
    return out


def noise_logits(n, seed=0, sigma=2.0):
    return np.random.default_rng(seed).normal(0, sigma, (n, 2)).astype(np.float32)
