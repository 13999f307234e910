"""The fact the Updated model's three inference schedules rest on (no GPU): the oracle's forward on full-neighbour 4-hop blocks gives, at the blocks'
targets, the rows of its forward on the whole-scene adjs of tests/updated_inference_model.py -- the model has no normalisation layer."""
import numpy as np
import pytest
import torch

from dgnn_amd.synthetic import delaunay_tet_graph, hashed_normal
from updated_inference_model import khop_blocks, make_clf, oracle_forward, oracle_net, oracle_whole_scene, whole_scene_adjs


def test_whole_scene_adjs_shape():
    ei = torch.tensor([[0, 1, 2, 2], [1, 0, 0, 1]])
    adjs = whole_scene_adjs(ei, 3, 4)
    assert len(adjs) == 4
    for a, e, s in adjs:
        assert a is ei and torch.equal(e, torch.arange(4)) and s == (3, 3)


@pytest.mark.parametrize("name,widths", [("sage", [16, 24, 24, 2]), ("sage+", [16, 24, 24, 24])])
def test_block_targets_equal_the_whole_scene_rows(name, widths):
    adj, _, _ = delaunay_tet_graph(300, seed=5)
    n = adj.shape[0] // 4
    ei = torch.from_numpy(adj.T.astype(np.int64))
    x = hashed_normal(np.arange(n), 29, seed=1).double()
    ea = hashed_normal(np.arange(4 * n), 3, seed=2).double()
    torch.manual_seed(3)
    net = oracle_net(28, make_clf(widths, name))
    whole = oracle_whole_scene(net, x, ea, ei)
    assert whole.dtype == torch.float64 and whole.shape == (n, 2)
    scale = max(1.0, whole.abs().max().item())
    seen = torch.zeros(n, dtype=torch.bool)
    for s in range(0, n, 97):
        batch = np.arange(s, min(s + 97, n))
        n_id, adjs = khop_blocks(ei, n, batch, net.num_layers)
        out = oracle_forward(net, x, ea, n_id, adjs)
        assert out.shape == (batch.size, 2)
        assert (out - whole[batch]).abs().max().item() <= 1e-12 * scale
        seen[batch] = True
    assert bool(seen.all())


@pytest.mark.parametrize("method", ["inference_layer", "inference_batch_layer", "inference_layer_batch"])
def test_inference_methods_refuse_a_cpu_device_like_forward(method):
    from dgnn_amd.config import Config
    from dgnn_amd.learning.surfaceNetUpdatedEdgeFilters import SurfaceNet
    net = SurfaceNet(28, make_clf([16, 24, 24, 24], "sage+", device="cpu"))
    data = Config(x=torch.zeros(4, 29), edge_attr=torch.zeros(16, 2), edge_index=torch.zeros(2, 16, dtype=torch.long),
                  n_id=torch.arange(4), adjs=whole_scene_adjs(torch.zeros(2, 16, dtype=torch.long), 4, 4))
    with pytest.raises(RuntimeError) as fwd:
        net(data)
    with pytest.raises(RuntimeError) as inf:
        getattr(net, method)(data) if method == "inference_layer" else getattr(net, method)(data, [])
    assert str(inf.value) == str(fwd.value)
