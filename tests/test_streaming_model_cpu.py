"""The fp64 restatements of streaming_model.py (BatchNorm1d chain, Adam) against independent references without a GPU: torch.nn.BatchNorm1d in
float64 followed by relu through autograd, torch.optim.Adam on float64 parameters, and the two-rank `count` form against the one-piece form.
Both sides are fp64 and differ in summation order only: every bound is 1e-10 times the magnitude terms of the quantity."""
import numpy as np
import pytest
import torch

import streaming_model as SM

TOL = 1e-10
EPS, MOM = 1e-5, 0.1


def bn_inputs(M, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, c, generator=g, dtype=torch.float64) * 2 + torch.randn(c, generator=g, dtype=torch.float64)
    x[:, 0] = 0.75                                                              # constant column: variance 0
    if c > 1:
        x[:, 1] = 1e3 + torch.randn(M, generator=g, dtype=torch.float64)        # mean 1e3, unit spread
    dy = torch.randn(M, c, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(c, generator=g, dtype=torch.float64) + 0.5, torch.randn(c, generator=g, dtype=torch.float64) * 0.3
    rm0, rv0 = torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    return x, dy, gamma, beta, rm0, rv0


def torch_bn(c, gamma, beta, rm0, rv0):
    bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=MOM).double()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    return bn


def close(got, want, mag):
    err = (got - want).abs()
    assert (err <= TOL * mag).all(), (err - TOL * mag).max().item()


@pytest.mark.parametrize("M,c", [(2, 5), (3, 1), (64, 28), (257, 96), (1000, 4)])
@pytest.mark.parametrize("relu", [True, False])
def test_bn_model_follows_batchnorm1d_in_train_mode(M, c, relu):
    x, dy, gamma, beta, rm0, rv0 = bn_inputs(M, c, 11 * M + c)
    bn = torch_bn(c, gamma, beta, rm0, rv0).train()
    xr = x.clone().requires_grad_(True)
    z = bn(xr)
    y = torch.relu(z) if relu else z
    y.backward(dy)
    mean, var, rm, rv = SM.bn_stats(x, rm0, rv0, MOM)
    assert var[0].item() <= 1e-25                                                # the constant column
    if c > 1 and M > 2:
        assert 0.05 < var[1].item() < 5.0                                        # the spread of the mean-1e3 column survives
    unb = var * M / (M - 1)
    close(rm, bn.running_mean, rm0.abs() + mean.abs())
    close(rv, bn.running_var, rv0.abs() + unb)
    scale, shift = SM.bn_fold(gamma, beta, mean, var, EPS)
    ym = x * scale + shift
    ym = torch.relu(ym) if relu else ym
    close(ym, y.detach(), x.abs() * scale.abs() + shift.abs())
    r = SM.bn_relu_bwd(x, ym, dy, gamma, mean, var, EPS, True, relu)
    # a mask that differs would be an O(1) difference; with the constant column BatchNorm's output is beta there on both sides
    assert torch.equal(ym > 0, y.detach() > 0)
    close(r.dbeta, bn.bias.grad, r.mag_dbeta)
    close(r.dgamma, bn.weight.grad, r.mag_dgamma)
    close(r.dx, xr.grad, r.mag_dx)


@pytest.mark.parametrize("M,c", [(1, 7), (2, 5), (257, 96)])
@pytest.mark.parametrize("relu", [True, False])
def test_bn_model_follows_batchnorm1d_in_eval_mode(M, c, relu):
    x, dy, gamma, beta, rm0, rv0 = bn_inputs(M, c, 13 * M + c)
    bn = torch_bn(c, gamma, beta, rm0, rv0).eval()
    xr = x.clone().requires_grad_(True)
    z = bn(xr)
    y = torch.relu(z) if relu else z
    y.backward(dy)
    scale, shift = SM.bn_fold(gamma, beta, rm0, rv0, EPS)
    ym = x * scale + shift
    ym = torch.relu(ym) if relu else ym
    close(ym, y.detach(), x.abs() * scale.abs() + shift.abs())
    assert torch.equal(ym > 0, y.detach() > 0)
    r = SM.bn_relu_bwd(x, ym, dy, gamma, rm0, rv0, EPS, False, relu)
    close(r.dx, xr.grad, r.mag_dx)
    close(r.dbeta, bn.bias.grad, r.mag_dbeta)
    close(r.dgamma, bn.weight.grad, r.mag_dgamma)
    assert torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0)


def test_bn_stats_of_a_single_row_keep_the_biased_variance():
    x, _, _, _, rm0, rv0 = bn_inputs(1, 6, 3)
    mean, var, rm, rv = SM.bn_stats(x, rm0, rv0, MOM)
    assert torch.equal(mean, x[0]) and torch.equal(var, torch.zeros(6, dtype=torch.float64))
    close(rv, (1 - MOM) * rv0, rv0)
    close(rm, (1 - MOM) * rm0 + MOM * x[0], rm0.abs() + x[0].abs())


def test_bn_fold_without_gamma_and_beta():
    _, _, _, _, mean, var = bn_inputs(4, 9, 5)
    scale, shift = SM.bn_fold(None, None, mean, var, EPS)
    close(scale, 1.0 / torch.sqrt(var + EPS), scale.abs())
    close(shift, -mean / torch.sqrt(var + EPS), shift.abs())


@pytest.mark.parametrize("M,cut", [(2, 1), (257, 1), (257, 85), (1000, 999)])
def test_count_form_on_two_pieces_gives_the_one_piece_backward(M, cut):
    c = 12
    x, dy, gamma, beta, rm0, rv0 = bn_inputs(M, c, 17 * M + cut)
    mean, var, _, _ = SM.bn_stats(x)
    scale, shift = SM.bn_fold(gamma, beta, mean, var, EPS)
    y = torch.relu(x * scale + shift)
    whole = SM.bn_relu_bwd(x, y, dy, gamma, mean, var, EPS, True, True)
    parts = [SM.bn_relu_bwd(x[a:b], y[a:b], dy[a:b], gamma, mean, var, EPS, True, True, count=M) for a, b in ((0, cut), (cut, M))]
    dbeta, dgamma = parts[0].dbeta + parts[1].dbeta, parts[0].dgamma + parts[1].dgamma
    close(dbeta, whole.dbeta, whole.mag_dbeta)
    close(dgamma, whole.dgamma, whole.mag_dgamma)
    dx = torch.cat([SM.bn_relu_bwd(x[a:b], y[a:b], dy[a:b], gamma, mean, var, EPS, True, True, count=M, sums=(dbeta, dgamma)).dx
                    for a, b in ((0, cut), (cut, M))])
    close(dx, whole.dx, whole.mag_dx)
    # a piece on its own sums and its own count is the one-piece form of that piece
    a = SM.bn_relu_bwd(x[:cut], y[:cut], dy[:cut], gamma, mean, var, EPS, True, True)
    b = SM.bn_relu_bwd(x[:cut], y[:cut], dy[:cut], gamma, mean, var, EPS, True, True, count=cut)
    assert torch.equal(a.dx, b.dx)


@pytest.mark.parametrize("lr,betas,eps", [(1e-3, (0.9, 0.999), 1e-8), (3e-2, (0.5, 0.9), 1e-6)])
def test_adam_model_follows_torch_adam_in_float64(lr, betas, eps):
    g = torch.Generator().manual_seed(7)
    shapes = [(5,), (64, 3), (1,), (300,)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps)
    mine = [(p.detach().numpy().copy(), np.zeros(s), np.zeros(s)) for p, s in zip(ps, shapes)]
    for t in range(1, 6):
        grads = [torch.randn(*s, generator=g, dtype=torch.float64) * 10.0 ** (3 * i - 6) for i, s in enumerate(shapes)]
        if t == 3:
            grads[1].zero_()
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
        mine = [SM.adam_step(p, gr.numpy(), m, v, lr, betas[0], betas[1], eps, t) for (p, m, v), gr in zip(mine, grads)]
        for (p, m, v), q in zip(mine, ps):
            st = opt.state[q]
            assert np.all(np.abs(m - st["exp_avg"].numpy()) <= TOL * np.abs(m) + 1e-300)
            assert np.all(np.abs(v - st["exp_avg_sq"].numpy()) <= TOL * v + 1e-300)
            step = lr / (1 - betas[0] ** t) * np.abs(m) / (np.sqrt(v) / np.sqrt(1 - betas[1] ** t) + eps)
            assert np.all(np.abs(p - q.detach().numpy()) <= TOL * (np.abs(p) + t * step))


def test_adam_f32_model_is_the_fp64_rule_at_fp32_rounding():
    """adam_step_f32 against adam_step from the same state: they differ by the ten-odd fp32 roundings of one step, and the host scalars are the
    double-precision values rounded once"""
    g = np.random.default_rng(5)
    f = np.float32
    p, m = g.standard_normal(4000).astype(f), (g.standard_normal(4000) * 1e-2).astype(f)
    v, gr = (g.standard_normal(4000) ** 2 * 1e-4).astype(f), (g.standard_normal(4000) * 1e-2).astype(f)
    lr, b1, b2, eps = (float(f(a)) for a in (1e-3, 0.9, 0.999, 1e-8))
    for t in (1, 7, 10000):
        a, b = SM.adam_host_scalars(lr, b1, b2, t)
        assert a == f(lr / (1 - b1 ** t)) and b == f(1 / np.sqrt(1 - b2 ** t))
        p32, m32, v32 = SM.adam_step_f32(p, gr, m, v, lr, b1, b2, eps, t)
        p64, m64, v64 = SM.adam_step(p, gr, m, v, lr, b1, b2, eps, t)
        u = 2.0 ** -24
        assert np.all(np.abs(m32 - m64) <= 4 * u * (np.abs(m) + np.abs(gr - m) * (1 - b1)))
        assert np.all(np.abs(v32 - v64) <= 4 * u * v64)
        assert np.all(np.abs(p32 - p64) <= u * np.abs(p64) + 16 * u * np.abs(p64 - p) + np.abs(m32 - m64) * (lr / (1 - b1 ** t)) / (np.sqrt(v64) / np.sqrt(1 - b2 ** t) + eps))
