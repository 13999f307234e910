"""Storage-rounding model of the Updated variant's TRAINING step in bf16 storage (test infrastructure; the training twin of
tests/test_bf16_rounding_model_cpu.py -- VERDICT r4 item 1b).

The reference step (learning/surfaceNetUpdatedEdgeFilters.py:147-176, 216-251 forward; autograd backward, learning/runModel.py:279) restated in fp64 on
the CPU with EXPLICIT forward and backward passes, so that a round-to-bf16 can be injected at exactly the tensors the HIP path stores or feeds to the
bf16 matrix cores (dgnn_amd/csrc/train.hip: updated_fwd / updated_bwd, dgnn_updated_stack_fwd / _bwd; bf16 twins of the generic kernels: widen on
load, fp32 arithmetic, round to nearest even on store):

  site "x"    the input rows x[n_id, 1:] cast once (functional._ToBF16) and layer 0's edge rows edge_attr[e_id, :2] (dgnn_cast_f32_to_bf16)
  site "w"    every fp32 master weight as it is staged into a bf16 matrix product (forward: We, Wl, Wr; backward: Wl^T, Wr^T, We^T)
  site "phi"  phi_l = lin_e(ea_l), written once in bf16 (read by the aggregation, by the next layer's lin_e through the chaining and by the backward)
  site "a"    a_l = mean_j x_j * phi, written by the aggregate kernel
  site "y"    y_l = relu?(lin_l(a) + lin_r(x_dst)), GEMM epilogue; the last layer's y are the logits (returned as y.float())
  site "dy"   the gradient arriving at the logits (autograd of y.float(): cast to bf16), every [da | dz.Wr] the input-gradient GEMM stores, every dx the
              aggregate backward stores (dx = agg_bwd(da, phi) + the stored dz.Wr, rounded once)
  site "dphi" dphi_l as the aggregate backward stores it, the sum dphi + dphi_ext (k_add_inplace), d_ea = dphi . We (the gradient the chaining hands to
              the previous layer's phi)

Weight GRADIENTS are fp32 accumulations of exact bf16 x bf16 products and are never rounded.  With every site off the function is the un-rounded
step: tests/test_bf16_rounding_model_cpu.py::test_training_model_without_rounding_is_the_oracle holds it to the oracle's autograd in fp64, which pins
this restatement.  With all sites on it is the yardstick the GPU gradients are compared with (tests/test_gpu_scale.py): whatever separates the HIP
path from THIS model beyond fp32-accumulation noise is a kernel bug; what separates this model from the un-rounded step is the price of the format
(BASELINE.md section 4).
"""
from __future__ import annotations

import torch

ALL_SITES = frozenset(("x", "w", "phi", "a", "y", "dy", "dphi"))


def _rb(t: torch.Tensor) -> torch.Tensor:
    """fp64 -> fp32 -> bf16 (round to nearest even twice: the GPU computes in fp32 and rounds on store) -> fp64"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def updated_step(sd, params, n_node_feat, x_all, edge_attr_all, n_id, adjs, G, sites=ALL_SITES, drop_col0=True, arith=torch.float64):
    """One forward + backward of the Updated "sage" model (no out_net) on one sampled block.
    sd: state dict (convs.{l}.lin_{e,l,r}.{weight,bias}); adjs[l] = (edge_index [2,E_l] local ids, e_id [E_l] rows of the scene's edge tensors,
    (n_src, n_dst)); loss = (logits * G).sum().  -> (logits fp64 [n_dst_last, params[-1]], {parameter name: gradient fp64})."""
    sites = frozenset(sites)
    R = {s: (_rb if s in sites else (lambda t: t)) for s in ALL_SITES}
    L = len(params)
    f64 = lambda t: t.detach().to("cpu", torch.float64).to(arith)
    P = {k: f64(v) for k, v in sd.items()}
    x = f64(x_all)[n_id.cpu()]
    x = R["x"](x[:, 1:] if drop_col0 else x)
    E_all = edge_attr_all.shape[0]
    saved = []
    ea = R["x"](f64(edge_attr_all)[adjs[0][1].cpu(), :2])
    for l in range(L):
        edge_index, e_id, size = adjs[l]
        src, dst, e_id = edge_index[0].cpu(), edge_index[1].cpu(), e_id.cpu()
        n_dst = int(size[1])
        We, be = P["convs.%d.lin_e.weight" % l], P["convs.%d.lin_e.bias" % l]
        Wl, bl, Wr = P["convs.%d.lin_l.weight" % l], P["convs.%d.lin_l.bias" % l], P["convs.%d.lin_r.weight" % l]
        c_in = Wl.shape[1]
        assert ea.shape[1] == We.shape[1] and x.shape[1] == c_in
        phi = R["phi"](ea @ R["w"](We).t() + be)                                              # :156
        cnt = torch.bincount(dst, minlength=n_dst).clamp(min=1).to(arith)
        S = torch.zeros((n_dst, c_in), dtype=arith).index_add_(0, dst, x[src] * phi)     # :158 (mean of x_j * phi)
        a = R["a"](S / cnt[:, None])
        z = a @ R["w"](Wl).t() + x[:n_dst] @ R["w"](Wr).t() + bl                                # :159-165
        relu = l < L - 1                                                                        # :239-241
        y = R["y"](torch.relu(z) if relu else z)
        p = None
        if l < L - 1:
            # :236-241 zeros[E_all, C]; [e_id] = phi; relu; the rows e_id_next the next layer reads (edge_in_{l+1} == this phi's width)
            pos = torch.full((E_all,), -1, dtype=torch.int64)
            pos[e_id] = torch.arange(e_id.numel())
            p = pos[adjs[l + 1][1].cpu()]
            ea_next = torch.where((p >= 0)[:, None], torch.relu(phi[p.clamp(min=0)]), torch.zeros((), dtype=arith))
        saved.append(dict(src=src, dst=dst, n_dst=n_dst, cnt=cnt, x=x, ea=ea, phi=phi, a=a, y=y, relu=relu, We=We, Wl=Wl, Wr=Wr, p_next=p))
        x = y
        if l < L - 1:
            ea = ea_next
    logits = x
    grads = {}
    g = R["dy"](f64(G))
    dphi_ext = None
    for l in range(L - 1, -1, -1):
        s = saved[l]
        dz = g * (s["y"] > 0) if s["relu"] else g
        grads["convs.%d.lin_l.weight" % l] = dz.t() @ s["a"]
        grads["convs.%d.lin_l.bias" % l] = dz.sum(0)
        grads["convs.%d.lin_r.weight" % l] = dz.t() @ s["x"][:s["n_dst"]]
        da = R["dy"](dz @ R["w"](s["Wl"]))                     # one GEMM against the stacked [Wl^T ; Wr^T]: both halves are stored in the storage type
        dxr = R["dy"](dz @ R["w"](s["Wr"]))
        dm = (da / s["cnt"][:, None])[s["dst"]]
        dphi = R["dphi"](dm * s["x"][s["src"]])
        if l > 0:
            dx = torch.zeros_like(s["x"]).index_add_(0, s["src"], dm * s["phi"])
            dx[:s["n_dst"]] += dxr
            dx = R["dy"](dx)
        if dphi_ext is not None:
            dphi = R["dphi"](dphi + dphi_ext)
        grads["convs.%d.lin_e.weight" % l] = dphi.t() @ s["ea"]
        grads["convs.%d.lin_e.bias" % l] = dphi.sum(0)
        dphi_ext = None
        if l > 0:
            d_ea = R["dphi"](dphi @ R["w"](s["We"]))
            prev = saved[l - 1]
            p = prev["p_next"]
            ok = p >= 0
            dphi_ext = torch.zeros_like(prev["phi"])
            dphi_ext[p[ok]] = d_ea[ok] * (prev["phi"][p[ok]] > 0)
            g = dx
    return logits.double(), {k: v.double() for k, v in grads.items()}


def error_table(ref, got):
    """{name: (max |d| / max |ref|, rms d / rms ref)}"""
    out = {}
    for k, r in ref.items():
        d = got[k].double().cpu() - r
        out[k] = (d.abs().max().item() / max(r.abs().max().item(), 1e-300), d.pow(2).mean().sqrt().item() / max(r.pow(2).mean().sqrt().item(), 1e-300))
    return out


# ---- the Static model (learning/surfaceNetStaticEdgeFilters.py, the project's main model) ------------------------------------------------------------
# Its bf16 training step runs layer by layer under autograd (train_step_direct and the whole-model calls decline bf16): functional._ToBF16, then per conv
# layer functional.sage_train_layer -> ops.sage_layer_train_fwd / _bwd -> csrc/train.hip dgnn_sage_layer_train_{fwd,bwd}_bf16, the decoder's
# Linear + BatchNorm + ReLU through the same call without a graph (rowptr NULL), and the output Linear as functional.linear2(out_f32=True).
# Where those kernels round (read in csrc/aggregate.hip k_agg_fwd / k_agg_bwd_c, gemm.hip k_linear_fwd_b / stage_w_bf16, norm.hip):
#
#   "x"      the input rows x[n_id, 1:] cast once (functional._ToBF16)
#   "w"      every fp32 weight staged into a bf16 matrix product: Wj, Wi, the decoder's W0, W3 forward; Wj^T, Wi^T, W0^T, W3^T backward
#   "a"      a = mean_j x_j * phi, stored by the aggregate (phi = ea . We^T + be is evaluated in fp32 registers from the fp32 edge rows: never rounded)
#   "z"      z = a . Wj^T + x_dst . Wi^T + bj (the decoder: x . W0^T + b0), the GEMM's store; the batch statistics are taken over THIS bf16 z
#   "y"      y = relu(z * scale + shift) of every BatchNorm (the conv layers' outputs and the decoder's hidden rows)
#   "dy"     the logits' gradient cast to bf16 where the output Linear's backward stages it (dh = g . W3 and dW3 = g^T h; db3 sums the fp32 g)
#   "dz"     dz of every BatchNorm's backward as dgnn_bn_relu_bwd_bf16 stores it (mask [y > 0] from the stored y)
#   "da"     da = dz . Wj stored ahead of the aggregate's backward
#   "dx"     every stored gradient of a layer's input rows: dh, the decoder block's dx = dz . W0, the aggregate backward's dx (fp32 sum, one rounding)
#   "dxacc"  the SECOND rounding of a conv layer's dx: dz . Wi^T is added in fp32 to the stored bf16 dx by the GEMM's DGNN_LINEAR_ACCUMULATE epilogue,
#            which rounds again (so dx[:n_dst] = bf16(bf16(aggregate part) + dz . Wi^T))
#
# Never rounded: edge_attr, We, be, phi, the BatchNorm statistics (fp64 sums on the device, fp32 mean / var / scale / shift), the running buffers
# and every parameter gradient (fp32 accumulations of exact bf16 x bf16 products; dWe / dbe from dphi = (da / deg) * x_j in fp32).
STATIC_SITES = frozenset(("x", "w", "a", "z", "y", "dy", "dz", "da", "dx", "dxacc"))
# The bound tests/test_gpu_scale.py::test_static_bf16_training_step_at_scale_matches_the_rounding_model holds the HIP gradients to (per tensor: rms of
# the difference / rms, largest entry of the difference / largest entry, rms along any one row or column / rms), set from the measured spread of this
# model in fp32 against fp64 (tests/test_bf16_rounding_model_cpu.py, which also checks the spread stays inside and which site families exceed it).
STATIC_BF16_RMS, STATIC_BF16_CAP, STATIC_BF16_LINE = 0.06, 0.3, 0.5


def _bn_train(z, gamma, beta, eps):
    """train-mode BatchNorm1d: batch mean, BIASED variance to normalise -> (out, x_hat, inv_std, mean, var)"""
    mean = z.mean(0)
    var = (z - mean).pow(2).mean(0)
    inv = 1.0 / torch.sqrt(var + eps)
    xh = (z - mean) * inv
    return xh * gamma + beta, xh, inv, mean, var


def _bn_relu_bwd(g, xh, inv, gamma):
    """backward of relu(BatchNorm_train(z)) given g = dy * [y > 0] -> (dz, dgamma, dbeta)"""
    M = g.size(0)
    dbeta = g.sum(0)
    dgamma = (g * xh).sum(0)
    return gamma * inv * (g - dbeta / M - xh * (dgamma / M)), dgamma, dbeta


def static_step(sd, convs, x_all, edge_attr_all, n_id, adjs, G, sites=STATIC_SITES, arith=torch.float64, drop_col0=True, momentum=0.1, eps=1e-5):
    """One training-mode forward + backward of the Static SurfaceNet (edge_convs 1, normalization 'b', decoder 2: the shipped configuration) on one
    sampled block, loss = (logits * G).sum(), with a round-to-bf16 at the `sites` above.  Restates reference :196-227 (oracle/static_edge_filters.py)
    and autograd's backward.  sd: state dict (convs.{l}.conv.lin_{e,j,i}, convs.{l}.norm.module.*, decoder.{0,1,3}.*); convs: the conv widths;
    adjs[l] = (edge_index [2, E_l] local ids, e_id [E_l] rows of edge_attr_all, (n_src, n_dst)); drop_col0: regularization.cell_type (_block_x).
    -> (logits [n_dst_last, 2], {parameter name: gradient}, {buffer name: value after the step}), all fp64 on the CPU."""
    sites = frozenset(sites)
    assert sites <= STATIC_SITES, sites - STATIC_SITES
    R = {s: (_rb if s in sites else (lambda t: t)) for s in STATIC_SITES}
    f = lambda t: t.detach().to("cpu", torch.float64).to(arith)
    P = {k: f(v) for k, v in sd.items() if v.is_floating_point()}
    L = len(convs)
    assert "decoder.3.weight" in P and "convs.%d.norm.module.weight" % (L - 1) in P, "static_step models decoder 2 with BatchNorm ('b') layers"
    x = f(x_all)[n_id.cpu()]
    x = R["x"](x[:, 1:] if drop_col0 else x)
    ea_all = f(edge_attr_all)
    bufs = {}

    def norm_fwd(pre, z):
        gamma, beta = P[pre + "weight"], P[pre + "bias"]
        out, xh, inv, mean, var = _bn_train(z, gamma, beta, eps)
        M = z.size(0)
        unb = var * (M / (M - 1)) if M > 1 else var          # csrc/norm.hip k_stats_finalize: one row keeps the biased value (0)
        bufs[pre + "running_mean"] = (1 - momentum) * P[pre + "running_mean"] + momentum * mean
        bufs[pre + "running_var"] = (1 - momentum) * P[pre + "running_var"] + momentum * unb
        bufs[pre + "num_batches_tracked"] = sd[pre + "num_batches_tracked"].detach().cpu() + 1
        return R["y"](torch.relu(out)), xh, inv

    saved = []
    for l in range(L):
        edge_index, e_id, size = adjs[l]
        src, dst, n_dst = edge_index[0].cpu(), edge_index[1].cpu(), int(size[1])
        p = "convs.%d." % l
        We, be = P[p + "conv.lin_e.weight"], P[p + "conv.lin_e.bias"]
        Wj, bj, Wi = P[p + "conv.lin_j.weight"], P[p + "conv.lin_j.bias"], P[p + "conv.lin_i.weight"]
        ea = ea_all[e_id.cpu()]
        phi = ea @ We.t() + be
        cnt = torch.bincount(dst, minlength=n_dst).clamp(min=1).to(arith)
        a = R["a"](torch.zeros((n_dst, x.size(1)), dtype=arith).index_add_(0, dst, x[src] * phi) / cnt[:, None])
        z = R["z"](a @ R["w"](Wj).t() + x[:n_dst] @ R["w"](Wi).t() + bj)
        y, xh, inv = norm_fwd(p + "norm.module.", z)
        saved.append(dict(src=src, dst=dst, n_dst=n_dst, cnt=cnt, x=x, ea=ea, phi=phi, a=a, y=y, xh=xh, inv=inv))
        x = y
    W0, b0, W3, b3 = P["decoder.0.weight"], P["decoder.0.bias"], P["decoder.3.weight"], P["decoder.3.bias"]
    z0 = R["z"](x @ R["w"](W0).t() + b0)
    h, xh0, inv0 = norm_fwd("decoder.1.module.", z0)
    logits = h @ R["w"](W3).t() + b3                          # fp32 out (linear2(out_f32=True)): not rounded

    grads = {}
    g = f(G)
    gb = R["dy"](g)
    grads["decoder.3.weight"] = gb.t() @ h
    grads["decoder.3.bias"] = g.sum(0)
    dh = R["dx"](gb @ R["w"](W3))
    dz, grads["decoder.1.module.weight"], grads["decoder.1.module.bias"] = _bn_relu_bwd(dh * (h > 0), xh0, inv0, P["decoder.1.module.weight"])
    dz = R["dz"](dz)
    grads["decoder.0.weight"] = dz.t() @ x
    grads["decoder.0.bias"] = dz.sum(0)
    dy = R["dx"](dz @ R["w"](W0))
    for l in range(L - 1, -1, -1):
        s, p = saved[l], "convs.%d." % l
        dz, grads[p + "norm.module.weight"], grads[p + "norm.module.bias"] = _bn_relu_bwd(dy * (s["y"] > 0), s["xh"], s["inv"], P[p + "norm.module.weight"])
        dz = R["dz"](dz)
        n_dst = s["n_dst"]
        grads[p + "conv.lin_j.weight"] = dz.t() @ s["a"]
        grads[p + "conv.lin_j.bias"] = dz.sum(0)
        grads[p + "conv.lin_i.weight"] = dz.t() @ s["x"][:n_dst]
        da = R["da"](dz @ R["w"](P[p + "conv.lin_j.weight"]))
        dm = (da / s["cnt"][:, None])[s["dst"]]
        dphi = dm * s["x"][s["src"]]
        grads[p + "conv.lin_e.weight"] = dphi.t() @ s["ea"]
        grads[p + "conv.lin_e.bias"] = dphi.sum(0)
        if l > 0:
            dx = R["dx"](torch.zeros_like(s["x"]).index_add_(0, s["src"], dm * s["phi"]))
            dx[:n_dst] = R["dxacc"](dx[:n_dst] + dz @ R["w"](P[p + "conv.lin_i.weight"]))
            dy = dx
    return logits.double(), {k: v.double() for k, v in grads.items()}, {k: (v.double() if v.is_floating_point() else v) for k, v in bufs.items()}
