"""The graph-cut oracle (tests/graph_cut_model.py) against brute-force enumeration, and its cost / weight conversions."""
import numpy as np
import pytest
import torch

import graph_cut_model as gcm


def _case(rng, n, f, sigma=2.0, ties=False):
    pred = rng.normal(0, sigma, (n, 2)).astype(np.float32)
    if ties:
        pred[::3, 1] = pred[::3, 0]                 # equal unary costs
        pred[1::4] = 0.0                            # costs of zero
    edges = rng.integers(0, n, (f, 2)).astype(np.int32)
    return pred, edges


@pytest.mark.parametrize("uw,bw", [(10, 1), (10, 10), (100, 100), (10.0, 10.0), (10, 0)])
def test_dinic_oracle_matches_brute_force(uw, bw):
    rng = np.random.default_rng(int(uw) * 1000 + int(bw))
    for trial in range(12):
        n = int(rng.integers(1, 15))
        pred, edges = _case(rng, n, int(rng.integers(0, 3 * n + 1)), ties=trial % 2 == 0)
        want, e_want = gcm.brute_force(pred, edges, uw, bw)
        got, e_got, flow = gcm.solve(pred, edges, uw, bw)
        assert np.array_equal(got, want) and e_got == e_want


def test_costs_are_the_reference_expression():
    pred = np.array([[0.05, 0.15], [0.25, -0.25], [1.0, 2.0], [-0.35, 0.45]], dtype=np.float32)
    D = gcm.unary_costs(pred, 10)
    ref = (torch.from_numpy(pred)[:, [1, 0]] * 10).round().numpy().astype(np.int64)
    assert np.array_equal(D, ref)
    # half to even on exact halves of the fp32 product: 0.25 * 10 = 2.5 -> 2, -0.25 * 10 = -2.5 -> -2
    assert D[1, 0] == -2 and D[1, 1] == 2


def test_potts_weight_truncates_like_numpy():
    assert gcm.potts_weight(10.0) == 10 and gcm.potts_weight(1) == 1 and gcm.potts_weight(2.9) == 2


def test_all_negative_costs_isolated_cells_duplicates_and_self_loops():
    pred = -np.abs(np.random.default_rng(3).normal(0, 3, (9, 2))).astype(np.float32)
    edges = np.array([[0, 1], [0, 1], [1, 1], [2, 3], [3, 2], [4, 4], [5, 6]], dtype=np.int32)   # 7, 8 isolated
    want, e_want = gcm.brute_force(pred, edges, 10, 10)
    got, e_got, _ = gcm.solve(pred, edges, 10, 10)
    assert np.array_equal(got, want) and e_got == e_want
