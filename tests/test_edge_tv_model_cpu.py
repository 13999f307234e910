"""The fp64 model of the edge total-variation regulariser (tests/edge_tv_model.py) against the values the REFERENCE's own learning/runModel.py
produced (tests/golden/trainer_f2.npz; 3e-6, the tolerance tests/test_reference_host_cpu.py holds the same quantities to), against torch autograd of
the fp64 op chain, and the condition on the seeded inputs of tests/test_gpu_edge_tv.py."""
import numpy as np
import pytest
import torch

import edge_tv_model as M
from helpers import gold

W = 0.37      # regularization.edge_weight of the fixture (test_reference_host_cpu.loss_clf)


def _branches(g):
    n_inner = int(g["reg_n_inner"])
    return (("batch", g["reg_logits"][:n_inner], g["reg_edge_index"]), ("whole", g["reg_logits"], g["reg_whole_edge_index"]))


def test_model_reproduces_the_reference_run():
    g = gold("trainer_f2.npz")
    _, kl_grad = M.kl_cell_loss(g["reg_logits"], g["batch_gt"], g["batch_x"][:, 0])
    kl_loss = float(g["total_early_batch"])
    for tag, logits, ei in _branches(g):
        m = M.edge_tv(logits, ei, W)
        want = float(g["reg_" + tag])
        assert abs(m["reg"] - want) <= 3e-6 * want, (tag, m["reg"], want)
        rs, es, rl = g["reg_metrics_" + tag]
        assert m["edges"] == es and abs(m["reg_sum"] - rs) <= 3e-6 * rs and abs(m["reg_sum"] / m["edges"] - rl) <= 3e-6 * rl
        assert abs(kl_loss + m["reg"] - float(g["total_" + tag])) <= 3e-6 * float(g["total_" + tag])
        share = g["total_grad_" + tag].astype(np.float64) - kl_grad          # the regulariser's share of the reference's total gradient
        got = np.zeros_like(share)
        got[:logits.shape[0]] = m["dlogits"]
        assert np.abs(got - share).max() <= 3e-6 * np.abs(g["total_grad_" + tag]).max(), (tag, np.abs(got - share).max())


@pytest.mark.parametrize("name", M.CASES)
def test_model_gradient_is_autograd_of_the_fp64_chain(name):
    logits, ei, _ = M.make_case(name)
    l = torch.from_numpy(logits).double().requires_grad_(True)
    e = torch.from_numpy(ei)
    inner = torch.softmax(l, dim=-1)
    tv = torch.abs(inner[e[0]][:, 0] - inner[e[1]][:, 0])
    reg = (tv * W).mean()
    (reg * 1.7).backward()
    m = M.edge_tv(logits, ei, W, g=1.7)
    assert abs(m["reg"] - reg.item()) <= 1e-12 and abs(m["reg_sum"] - (tv * W).sum().item()) <= 1e-12 * max(1.0, m["reg_sum"])
    assert np.abs(m["dlogits"] - l.grad.numpy()).max() <= 1e-12


@pytest.mark.parametrize("name", M.CASES)
def test_seeded_inputs_keep_every_edge_away_from_a_sign_flip(name):
    """apart from the deliberate exact ties no edge has 0 < |p(s) - p(d)| < 1e-5 in fp64 (fp32 evaluates p to ~1e-7), and the spread is >= 1"""
    logits, ei, ties = M.make_case(name)
    M.assert_separated(logits, ei, ties)
    if logits.shape[0] > 1:
        assert logits.std() >= 1.0
    if name.startswith("large"):
        assert (ei[1] == 123).sum() >= 5000 and ei.shape[1] % 4 == (0 if name == "large_aligned" else 3)
    if name == "tiny":
        assert not (ei == 4).any() and (logits[2] == logits[3]).all() and ((ei[0] == 0) & (ei[1] == 1)).sum() == 2


def test_saturated_rows_are_finite_with_zero_gradient():
    logits = np.array([[200.0, 0.0], [0.0, 200.0], [0.5, -0.5], [-300.0, 300.0]], np.float32)
    ei = np.array([[0, 1, 2, 3], [1, 2, 0, 0]], np.int64)
    m = M.edge_tv(logits, ei, W)
    assert np.isfinite(m["reg"]) and np.isfinite(m["dlogits"]).all()
    assert np.abs(m["dlogits"][[0, 1, 3]]).max() < 1e-80          # (fp64 still holds exp(-200); fp32 does not: exactly 0 on the device)
