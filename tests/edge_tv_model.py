"""fp64 statement of the edge total-variation regulariser and its gradient (numpy), the yardstick of csrc/edge_tv.hip:

    p(v) = softmax(logits_v)_0,  tv_e = |p(s_e) - p(d_e)|,  reg = w * sum_e tv_e / E,  metric sums (w * sum_e tv_e, E)
    c(v) = sum_{s_e = v} sgn_e - sum_{d_e = v} sgn_e,  sgn_e = sign(p(s_e) - p(d_e)), sign(0) = 0
    dlogits_v = g * (w / E) * c(v) * p(v) (1 - p(v)) * (+1, -1)

and of the volume-weighted KL cell loss's gradient (cell_norm none), which the reference-run totals contain next to it."""
import numpy as np


def inside_prob(logits):
    """p(v) without overflow for any logit difference: 1 / (1 + exp(l1 - l0)) split by sign"""
    l = np.asarray(logits, dtype=np.float64)
    d = l[:, 1] - l[:, 0]
    e = np.exp(-np.abs(d))
    return np.where(d >= 0, e / (1 + e), 1 / (1 + e)), e / (1 + e) ** 2      # p, p (1 - p)


def edge_tv(logits, edge_index, weight, g=1.0):
    """-> dict(reg, reg_sum, edges, dlogits [n, 2], c [n] = the signed edge counts, diff [E] = p(s_e) - p(d_e))"""
    ei = np.asarray(edge_index).astype(np.int64)
    src, dst = ei[0], ei[1]
    E = src.shape[0]
    p, pq = inside_prob(logits)
    diff = p[src] - p[dst]
    tv_sum = np.abs(diff).sum()
    sgn = np.sign(diff)
    c = np.zeros(p.shape[0])
    np.add.at(c, src, sgn)
    np.add.at(c, dst, -sgn)
    d0 = g * (weight / E) * c * pq
    return dict(reg=weight * tv_sum / E, reg_sum=weight * tv_sum, edges=E, dlogits=np.stack([d0, -d0], 1), c=c.astype(np.int64), diff=diff)


def kl_cell_loss(logits, gt, vol):
    """-> (loss, dlogits) of sum_k w_k sum_c kl_div(log_softmax(logits_k)_c, gt_kc) / sum_k w_k with w = vol"""
    l, t, w = np.asarray(logits, np.float64), np.asarray(gt, np.float64)[:, :2], np.asarray(vol, np.float64)
    m = l.max(1, keepdims=True)
    lsm = (l - m) - np.log(np.exp(l - m).sum(1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        cell = np.where(t > 0, t * (np.log(t) - lsm), 0.0).sum(1)
    loss = (cell * w).sum() / w.sum()
    return loss, (w / w.sum())[:, None] * (np.exp(lsm) * t.sum(1, keepdims=True) - t)


def well_separated_logits(n, edge_index, seed, tie_rows=(), spread=2.0, gap=1e-5):
    """fp32 logits [n, 2] from a fixed seed such that, apart from `tie_rows` (pairs of rows made bitwise equal), no edge has
    0 < |p(s) - p(d)| < gap in fp64: the fp32 sign of an edge cannot then legitimately differ from the model's.  Rows that violate it are redrawn."""
    rng = np.random.default_rng(seed)
    l = (rng.standard_normal((n, 2)) * spread).astype(np.float32)
    for a, b in tie_rows:
        l[b] = l[a]
    ei = np.asarray(edge_index).astype(np.int64)
    fixed = {r for ab in tie_rows for r in ab}
    for _ in range(100):
        p, _ = inside_prob(l)
        d = np.abs(p[ei[0]] - p[ei[1]])
        bad = (d > 0) & (d < gap)
        if not bad.any():
            return l
        rows = sorted(set(ei[0][bad].tolist()) - fixed) or sorted(set(ei[1][bad].tolist()) - fixed)
        l[rows] = (rng.standard_normal((len(rows), 2)) * spread).astype(np.float32)
    raise AssertionError("no well-separated draw")


def assert_separated(logits, edge_index, ties=0, gap=1e-5):
    """the condition on the inputs: exactly `ties` edges between distinct nodes with p(s) == p(d) (the deliberate ones), none with 0 < |diff| < gap"""
    ei = np.asarray(edge_index).astype(np.int64)
    p, _ = inside_prob(logits)
    d = np.abs(p[ei[0]] - p[ei[1]])
    assert not ((d > 0) & (d < gap)).any(), d[(d > 0) & (d < gap)]
    assert int(((d == 0) & (ei[0] != ei[1])).sum()) == ties


CASES = ("self_loop", "tiny", "remainders", "large", "large_aligned")


def make_case(name):
    """-> (logits fp32 [n, 2], edge_index int64 [2, E], number of deliberate tie edges) of the shapes the kernels are held to:
    self_loop  n 1, E 1: tv = 0, gradient 0
    tiny       n 5, E 7: a repeated edge, node 4 on no edge, rows 2 and 3 bitwise equal and joined by an edge (sign 0)
    remainders n 257, E 1031: crosses the 64-lane and 256-thread boundaries with remainders
    large      n 70 001, E 280 003: node 123 is the dst of 5 000 edges (the integer atomics)
    large_aligned  the same with E 280 004: both rows of a contiguous [2, E] tensor are 16-byte aligned for int32 and int64 (the two-row vector form)"""
    if name == "self_loop":
        return np.array([[0.3, -1.2]], np.float32), np.zeros((2, 1), np.int64), 0
    if name == "tiny":
        ei = np.array([[0, 0, 1, 2, 3, 1, 0], [1, 1, 2, 3, 0, 3, 2]], np.int64)
        return well_separated_logits(5, ei, 11, tie_rows=[(2, 3)]), ei, 1
    n, E = {"remainders": (257, 1031), "large": (70001, 280003), "large_aligned": (70001, 280004)}[name]
    rng = np.random.default_rng(E)
    ei = rng.integers(0, n, (2, E)).astype(np.int64)
    if name.startswith("large"):
        ei[1, 1000:6000] = 123
    return well_separated_logits(n, ei, E + 1), ei, 0
