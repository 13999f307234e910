"""fp64 restatement (plain torch, CPU) of the reference Static SurfaceNet with ``normalization: l`` -- PyG 2.0.2's graph LayerNorm
(one mean / one biased std over all rows of the call, eps on the std) after every conv layer, inside the decoder and inside the
two-layer edge filter -- and of the reference's three schedules (learning/surfaceNetStaticEdgeFilters.py:196-355).  Parameters are a
dict name -> tensor with the checkpoint keys; nothing here touches the GPU."""
from __future__ import annotations

import torch


def pyg_layer_norm(x, w, b, eps=1e-5):
    x = x - x.mean()
    out = x / (x.std(unbiased=False) + eps)
    return out * w + b


def _lin(x, p, name, bias=True):
    y = x @ p[name + ".weight"].t()
    return y + p[name + ".bias"] if bias else y


def num_layers(p):
    return len({k.split(".")[1] for k in p if k.startswith("convs.")})


def edge_convs(p):
    return 2 if "convs.0.conv.lin_e.1.weight" in p else 1


def decoder_depth(p):
    return 2 if "decoder.3.weight" in p else 1


def edge_filter(p, i, ea):
    pre = "convs.%d.conv.lin_e" % i
    if edge_convs(p) == 1:
        return _lin(ea, p, pre)
    h = torch.relu(pyg_layer_norm(_lin(ea, p, pre + ".0"), p[pre + ".1.weight"], p[pre + ".1.bias"]))
    return _lin(h, p, pre + ".3")


def conv(p, i, x_src, x_dst, ea, ei):
    """mean_j x_j * lin_e(e_ji) -> lin_j, + lin_i(x_dst) (reference :66-87 with PyG's mean aggregation, count clamped to 1)"""
    msg = x_src[ei[0]] * edge_filter(p, i, ea)
    n_dst = x_dst.size(0)
    s = torch.zeros((n_dst, msg.size(1)), dtype=msg.dtype).index_add(0, ei[1], msg)
    cnt = torch.zeros(n_dst, dtype=msg.dtype).index_add(0, ei[1], torch.ones(ei.size(1), dtype=msg.dtype)).clamp(min=1)
    pre = "convs.%d.conv" % i
    return _lin(s / cnt[:, None], p, pre + ".lin_j") + _lin(x_dst, p, pre + ".lin_i", bias=False)


def layer(p, i, x_src, x_dst, ea, ei):
    return torch.relu(pyg_layer_norm(conv(p, i, x_src, x_dst, ea, ei), p["convs.%d.norm.weight" % i], p["convs.%d.norm.bias" % i]))


def decoder(p, x):
    if decoder_depth(p) == 1:
        return _lin(x, p, "decoder.0")
    h = torch.relu(pyg_layer_norm(_lin(x, p, "decoder.0"), p["decoder.1.weight"], p["decoder.1.bias"]))
    return _lin(h, p, "decoder.3")


def inference_layer(p, x, ea, ei):
    """x with the loss-weight column 0 (cell_type 'vol': dropped, reference :329-332)"""
    x = x[:, 1:]
    for i in range(num_layers(p)):
        x = layer(p, i, x, x, ea, ei)
    return decoder(p, x)


def forward_blocks(p, x_all, ea_all, n_id, adjs):
    """train forward (reference :196-227) on sampled blocks [(edge_index, e_id, (n_src, n_dst))]"""
    x = x_all[n_id, 1:]
    for i in range(num_layers(p)):
        ei, e_id, size = adjs[i]
        x = layer(p, i, x, x[:size[1]], ea_all[e_id], ei)
    return decoder(p, x)


def inference_batch_layer(p, x_all, ea_all, loader):
    """reference :232-275: every batch's k-hop blocks through all layers and the decoder, LayerNorm statistics per batch and layer"""
    out = torch.zeros((x_all.size(0), 2), dtype=x_all.dtype)
    for batch_size, n_id, adjs in loader:
        out[n_id[:batch_size]] = forward_blocks(p, x_all, ea_all, n_id, adjs)
    return out


def inference_layer_batch(p, x_all, ea_all, loader):
    """reference :279-320: layer by layer over 1-hop batches (statistics per batch), the decoder over the concatenated scene"""
    x = x_all[:, 1:]
    for i in range(num_layers(p)):
        xs = []
        for batch_size, n_id, (ei, e_id, size) in loader:
            h = x[n_id]
            xs.append(layer(p, i, h, h[:size[1]], ea_all[e_id], ei))
        x = torch.cat(xs, 0)
    return decoder(p, x)


def params64(sd, requires_grad=False):
    return {k: torch.as_tensor(v).double().clone().requires_grad_(requires_grad) for k, v in sd.items()}
