#!/usr/bin/env python3
"""Generates tests/golden/static_ln_*.npz by RUNNING THE REFERENCE's Static SurfaceNet with ``normalization: l``.

Run in the authoring container only (needs the reference tree, like make_golden.py):

    python tests/golden/make_golden_ln.py

It reuses make_golden.py's stand-in packages, with one entry replaced: ``torch_geometric.nn.norm`` gets a
``LayerNorm`` that states our reading of PyG 2.0.2's graph LayerNorm for ``batch=None`` (the branch the reference
takes at surfaceNetStaticEdgeFilters.py:165,173,185 and in the edge filter :134):

    x = x - x.mean()                              # one scalar mean over all M*C elements
    out = x / (x.std(unbiased=False) + eps)       # eps added to the std
    out = out * weight + bias                     # weight [C] (init 1), bias [C] (init 0), no buffers

Then the UNMODIFIED reference SurfaceNet runs on a small seeded Delaunay scene with widths [32, 64, 40], decoder 2,
randomised LayerNorm weights and biases, edge_convs 1 and 2:
* static_ln_scene.npz: the scene (x, edge_attr, adjacencies) and the 3-hop training blocks of 24 target cells
* static_ln_e{1,2}.npz: the parameters, inference_layer logits in fp32 and fp64, the train-mode forward logits on
  the blocks, the upstream gradient G and every parameter's gradient of sum(logits * G).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

mg.STANDIN["torch_geometric/nn/norm/__init__.py"] = """
    import torch
    class BatchNorm(torch.nn.Module):
        def __init__(self, in_channels, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
            super().__init__()
            self.module = torch.nn.BatchNorm1d(in_channels, eps, momentum, affine, track_running_stats)
        def forward(self, x): return self.module(x)
    class LayerNorm(torch.nn.Module):
        # PyG 2.0.2 torch_geometric.nn.norm.LayerNorm, batch=None branch
        def __init__(self, in_channels, eps=1e-5, affine=True):
            super().__init__()
            self.in_channels, self.eps = in_channels, eps
            if affine:
                self.weight = torch.nn.Parameter(torch.ones(in_channels))
                self.bias = torch.nn.Parameter(torch.zeros(in_channels))
            else:
                self.register_parameter('weight', None)
                self.register_parameter('bias', None)
        def forward(self, x, batch=None):
            assert batch is None
            x = x - x.mean()
            out = x / (x.std(unbiased=False) + self.eps)
            if self.weight is not None and self.bias is not None:
                out = out * self.weight + self.bias
            return out
"""

CONVS = [32, 64, 40]


def ln_clf(edge_convs):
    clf = mg.static_clf()
    clf.model.convs = list(CONVS)
    clf.model.edge_convs = edge_convs
    clf.model.decoder = 2
    clf.model.normalization = "l"
    return clf


def main():
    torch.set_num_threads(1)
    ref = mg.load_ref()
    from dgnn_amd.synthetic import delaunay_tet_graph
    from oracle.pyg_semantics import neighbor_sampler_full  # restated NeighborSampler (see its docstring)
    adj, _, _ = delaunay_tet_graph(100, seed=41)
    n = adj.shape[0] // 4
    ei = adj.T.astype(np.int64)
    g = torch.Generator().manual_seed(41)
    x = torch.randn(n, 29, generator=g)
    x[:, 0] = x[:, 0].abs() + 0.1
    ea = torch.randn(4 * n, 20, generator=g)
    rng = np.random.default_rng(41)
    batch = rng.choice(n, size=24, replace=False)
    n_id, adjs = neighbor_sampler_full(ei, n, batch, len(CONVS))
    scene = dict(x=x.numpy(), edge_attr=ea.numpy(), adjacencies=adj, batch=batch.astype(np.int64), n_id=n_id, convs=np.asarray(CONVS))
    for i, (a, e, s) in enumerate(adjs):
        scene["adj%d_edge_index" % i] = a
        scene["adj%d_e_id" % i] = e
        scene["adj%d_size" % i] = np.asarray(s, np.int64)
    np.savez_compressed(os.path.join(HERE, "static_ln_scene.npz"), **scene)

    for e in (1, 2):
        clf = ln_clf(e)
        torch.manual_seed(100 + e)
        net = ref["surfaceNetStaticEdgeFilters"].SurfaceNet(clf)
        n_ln = 0
        with torch.no_grad():
            for m in net.modules():
                if type(m).__name__ == "LayerNorm":
                    m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape))
                    m.bias.copy_(0.2 * torch.randn(m.bias.shape))
                    n_ln += 1
        assert n_ln == len(CONVS) + 1 + (len(CONVS) if e == 2 else 0), n_ln
        out = {"param." + k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
        net.eval()
        with torch.no_grad():
            out["logits"] = net.inference_layer(mg.AD(x=x, edge_attr=ea, edge_index=torch.from_numpy(ei))).numpy()
            net64 = ref["surfaceNetStaticEdgeFilters"].SurfaceNet(clf)
            net64.load_state_dict(net.state_dict())
            net64 = net64.double().eval()
            out["logits64"] = net64.inference_layer(mg.AD(x=x.double(), edge_attr=ea.double(), edge_index=torch.from_numpy(ei))).numpy()
        net.train()
        data = mg.AD(all=mg.AD(x=x, edge_attr=ea), batch_n_id=torch.from_numpy(n_id),
                     batch_adjs=[(torch.from_numpy(a), torch.from_numpy(e_), s) for a, e_, s in adjs])
        logits = net(data)
        G = torch.randn(logits.shape, generator=g)
        (logits * G).sum().backward()
        out["train_logits"] = logits.detach().numpy()
        out["G"] = G.numpy()
        for k, p in net.named_parameters():
            out["grad." + k] = p.grad.numpy()
        np.savez_compressed(os.path.join(HERE, "static_ln_e%d.npz" % e), **out)
        print("edge_convs %d: cells %d, |logits| max %.3f, fp32 vs fp64 %.2e" % (e, n, np.abs(out["logits"]).max(),
                                                                                np.abs(out["logits"] - out["logits64"]).max()))


if __name__ == "__main__":
    main()
