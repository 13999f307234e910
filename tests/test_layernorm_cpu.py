"""normalization 'l' (PyG graph LayerNorm) without a GPU: the Static SurfaceNet builds with the reference's state-dict layout, the
fp64 restatement in layernorm_model.py reproduces the reference run recorded in tests/golden/static_ln_*.npz, and the library
declares the LayerNorm entry points."""
import os
import re

import numpy as np
import pytest
import torch

import layernorm_model as R
from dgnn_amd.config import reconbench_pretrained

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def gold(name):
    return np.load(os.path.join(HERE, "golden", name))


def ln_clf(edge_convs=1, decoder=2, convs=(32, 64, 40), device="cpu"):
    clf = reconbench_pretrained(device=device, convs=convs)
    clf.model.normalization = "l"
    clf.model.edge_convs = edge_convs
    clf.model.decoder = decoder
    return clf


@pytest.mark.parametrize("edge_convs", [1, 2])
def test_static_surfacenet_builds_with_layernorm_and_pyg_keys(edge_convs):
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import LayerNorm, SurfaceNet
    net = SurfaceNet(ln_clf(edge_convs, convs=(64, 128, 128, 128)))
    sd = net.state_dict()
    for i, c in enumerate((64, 128, 128, 128)):
        assert isinstance(net.convs[i][1], LayerNorm)
        assert tuple(sd["convs.%d.norm.weight" % i].shape) == (c,) and tuple(sd["convs.%d.norm.bias" % i].shape) == (c,)
        assert torch.equal(sd["convs.%d.norm.weight" % i], torch.ones(c)) and torch.equal(sd["convs.%d.norm.bias" % i], torch.zeros(c))
        if edge_convs == 2:
            assert tuple(sd["convs.%d.conv.lin_e.1.weight" % i].shape) == (40,) and tuple(sd["convs.%d.conv.lin_e.1.bias" % i].shape) == (40,)
    assert tuple(sd["decoder.1.weight"].shape) == (64,) and tuple(sd["decoder.1.bias"].shape) == (64,)
    assert not any("running" in k or "num_batches" in k for k in sd)          # no buffers
    ln = net.decoder[1]
    assert ln.in_channels == 64 and ln.eps == 1e-5


@pytest.mark.parametrize("edge_convs", [1, 2])
def test_fixture_state_dict_loads_into_the_model(edge_convs):
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import SurfaceNet
    g = gold("static_ln_e%d.npz" % edge_convs)
    sd = {k[len("param."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param.")}
    net = SurfaceNet(ln_clf(edge_convs))
    assert str(net.load_state_dict(sd)) == "<All keys matched successfully>"


@pytest.mark.parametrize("edge_convs", [1, 2])
def test_fp64_restatement_reproduces_the_reference_run(edge_convs):
    s, g = gold("static_ln_scene.npz"), gold("static_ln_e%d.npz" % edge_convs)
    p = R.params64({k[len("param."):]: g[k] for k in g.files if k.startswith("param.")}, requires_grad=True)
    x, ea = torch.from_numpy(s["x"]).double(), torch.from_numpy(s["edge_attr"]).double()
    ei = torch.from_numpy(s["adjacencies"].T.astype(np.int64))
    with torch.no_grad():
        lg = R.inference_layer(p, x, ea, ei)
    assert np.abs(lg.numpy() - g["logits64"]).max() <= 1e-10
    assert np.abs(lg.numpy() - g["logits"]).max() <= 1e-5
    adjs = [(torch.from_numpy(s["adj%d_edge_index" % i]), torch.from_numpy(s["adj%d_e_id" % i]), tuple(int(v) for v in s["adj%d_size" % i]))
            for i in range(3)]
    tl = R.forward_blocks(p, x, ea, torch.from_numpy(s["n_id"]), adjs)
    assert np.abs(tl.detach().numpy() - g["train_logits"]).max() <= 1e-5
    (tl * torch.from_numpy(g["G"]).double()).sum().backward()
    for k, t in p.items():
        ref = g["grad." + k]
        assert np.linalg.norm(t.grad.numpy() - ref) <= 1e-5 * max(np.linalg.norm(ref), 1e-3), k


def test_pyg_layer_norm_semantics():
    """one scalar mean / std over the whole tensor, eps on the std, constant input -> bias"""
    x = torch.randn(7, 3, dtype=torch.float64)
    w, b = torch.rand(3, dtype=torch.float64), torch.rand(3, dtype=torch.float64)
    y = R.pyg_layer_norm(x, w, b)
    m, sd = x.mean(), ((x - x.mean()) ** 2).mean().sqrt()
    assert torch.allclose(y, (x - m) / (sd + 1e-5) * w + b)
    assert torch.equal(R.pyg_layer_norm(torch.full((5, 3), 2.5, dtype=torch.float64), w, b), b.expand(5, 3))


def test_header_and_binding_declare_the_layernorm_entry_points():
    from dgnn_amd._lib import SIGNATURES
    src = open(os.path.join(ROOT, "include", "dgnn_hip.h")).read()
    for name in ("dgnn_graph_ln_stats", "dgnn_graph_ln_finalize_fold", "dgnn_graph_ln_apply", "dgnn_graph_ln_relu_bwd", "dgnn_graph_ln_stats_blocks",
                 "dgnn_graph_ln_scratch_elems"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in SIGNATURES, name
    assert "lnorm.hip" in open(os.path.join(ROOT, "dgnn_amd", "csrc", "Makefile")).read()


def test_host_queries_of_the_layernorm_library():
    from dgnn_amd._lib import LIB_PATH, lib
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g_
        g_.build()
    l = lib()
    assert l.dgnn_graph_ln_stats_blocks(0, 4) == 0
    assert l.dgnn_graph_ln_stats_blocks(1, 4) == 1 and l.dgnn_graph_ln_stats_blocks(10 ** 7, 128) == 1024
    # backward scratch holds the column partials [blocks][2][c] as doubles
    assert l.dgnn_graph_ln_scratch_elems(10 ** 6, 128) >= 1024 * 2 * 128 * 2


def test_layernorm_model_refuses_bf16_storage_and_partitioned_scene():
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import SurfaceNet
    from dgnn_amd.partition import PartitionedScene
    net = SurfaceNet(ln_clf())
    with pytest.raises(NotImplementedError):
        net.set_storage_dtype(torch.bfloat16)
    assert net.set_storage_dtype(torch.float32) is net
    scene = PartitionedScene.__new__(PartitionedScene)
    with pytest.raises(NotImplementedError):
        scene.inference_layer(net)
    with pytest.raises(NotImplementedError):
        scene.train_forward(net)
