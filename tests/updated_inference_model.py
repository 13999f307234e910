"""Test-side statement of whole-scene inference with the Updated SurfaceNet (what SurfaceNet.inference_* of surfaceNetUpdatedEdgeFilters compute).

The logits of a scene ``(x, edge_attr, edge_index)`` are what ``oracle.updated_edge_filters.SurfaceNet.forward`` returns in eval mode for
``n_id = arange(N)`` and ``adjs = [(edge_index, arange(E), (N, N))] * num_layers``: every layer sees the whole graph, every ``e_id`` is the identity,
and the reference's edge chaining (``zeros[E_all, C]; [e_id] = phi; relu; [e_id, :k]``) is ``ea_{k+1} = relu(phi_k)[:, :k]``.  The model has no
normalisation layer, so the full-neighbour k-hop blocks of a batch give the same rows at the batch's targets (tests/test_updated_inference_model_cpu.py):
the fact the three inference schedules rest on.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from dgnn_amd.config import Config


def whole_scene_adjs(edge_index: torch.Tensor, n: int, num_layers: int):
    """the `adjs` of a whole scene: one (edge_index, arange(E), (N, N)) per layer"""
    e_id = torch.arange(edge_index.size(1), dtype=torch.int64)
    return [(edge_index, e_id, (int(n), int(n)))] * int(num_layers)


def make_clf(model_params, model_name, device="cpu", drop_col0=True):
    return Config.wrap(dict(training=dict(model_params=[int(v) for v in model_params], model_name=model_name, loss="kl"),
                            features=dict(normalization_feature=1 if drop_col0 else 0, keep_normalization_feature=0), temp=dict(device=device),
                            inference=dict(batch_size=0, per_layer=1, has_label=0), regularization=dict(cell_type=None, cell_norm=None, edge_type=None)))


@contextlib.contextmanager
def default_dtype(dtype):
    """the oracle's forward allocates its [E_all, C] edge tensor in the default dtype: an fp64 run needs fp64 there too"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def oracle_net(n_features, clf, state_dict=None, dtype=torch.float64):
    from oracle.updated_edge_filters import SurfaceNet
    net = SurfaceNet(n_features, clf)
    if state_dict is not None:
        net.load_state_dict(state_dict)
    return net.to(dtype).eval()


def oracle_forward(net, x, edge_attr, n_id, adjs, dtype=torch.float64):
    with torch.no_grad(), default_dtype(dtype):
        return net(Config(x=x.to(dtype), edge_attr=edge_attr.to(dtype), n_id=n_id, adjs=adjs))


def oracle_whole_scene(net, x, edge_attr, edge_index, dtype=torch.float64):
    n = x.size(0)
    return oracle_forward(net, x, edge_attr, torch.arange(n), whole_scene_adjs(edge_index, n, net.num_layers), dtype)


def khop_blocks(edge_index: torch.Tensor, n: int, batch, hops: int):
    """(n_id, adjs) of one batch as PyG's NeighborSampler(sizes=[-1] * hops) builds them (oracle.pyg_semantics.neighbor_sampler_full)"""
    from oracle.pyg_semantics import neighbor_sampler_full
    n_id, adjs = neighbor_sampler_full(edge_index.numpy(), n, np.asarray(batch, dtype=np.int64), hops)
    return torch.from_numpy(n_id), [(torch.from_numpy(ei), torch.from_numpy(e), s) for ei, e, s in adjs]
