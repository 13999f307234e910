"""Feature scaling on the device (dgnn_scale_features_f64, ops.scale_features, dataLoader.run) against
* tests/golden/ingest_scalers.npz: the reference's own dataLoader on tests/golden/scene_small, one entry per route;
* the numpy model (tests/ingest_scalers_model.py) on synthetic fp64 frames at the smallest shapes where the selection and the
  merges can go wrong.

Bounds.  Outputs: |d| <= 1e-6 * max(1, |want|) (one fp32 ulp is <= 6e-8 |want|; the fp64 statistics differ by summation order only).
Selected statistics (robust centre and IQR, min-max min and range) without pre-steps: equal to the bit -- they are values of the
column, or one or two fp64 operations on such values, the same operations the model performs.  Summed statistics (the standard
scaler's, and everything behind a column sum): |d| <= 1e-12 * |want|, each statistic against itself.  The device sums 512 blocks of
4 row phases in a fixed order, the model row after row; on these frames the two orders differ by at most 6e-13 of the statistic (the
sum-scaled columns at n = 70 001), and no column of the frames cancels to a mean without digits of its own.
Elements that are equal (two infinities of one sign: a 1e300 column cast to fp32) are in bound.
"""
import json
import os

import numpy as np
import pytest
import torch

import ingest_scalers_model as M
from dgnn_amd.config import Config, reconbench_pretrained
from helpers import gold, kf96_state_dict, oracle_static

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL_LOGIT = 1e-4          # tests/test_gpu_parity.py
SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_small")
SCENE_D = dict(path=SCENE, filename="0", category="", id="", scan_conf="", gtfile="gt/0", ioufile="")
G = gold("ingest_scalers.npz")
CONFIGS = [(name, ov) for name, ov in json.loads(str(G["configs"]))]


def clf_for(overrides):
    clf = reconbench_pretrained(device=DEV)
    for k, v in overrides.items():
        sec, key = k.split(".")
        clf[sec][key] = v
    clf.temp.cell_order = "none"
    return clf


def out_err(got, want):
    """largest |d| / max(1, |want|) over the elements that are not equal"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    with np.errstate(invalid="ignore"):
        e = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    e[got == want] = 0.0
    return float(e.max()) if e.size else 0.0          # (a NaN -- an infinity against a number -- compares false below)


def stat_err(got, want, norm):
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(got - want) / norm
    e[got == want] = 0.0
    return float(e.max()) if e.size else 0.0


# ---- 1. the loader against the reference's loader --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in CONFIGS])
def test_loader_matches_reference_loader(name):
    from dgnn_amd.processing.data import dataLoader
    clf = clf_for(dict(CONFIGS)[name])
    dl = dataLoader(clf, verbosity=0)
    dl.run(SCENE_D)
    assert dl.features.is_cuda and dl.features.dtype == torch.float32 and dl.edge_features.dtype == torch.float32 and dl.cell_order is None
    wf, we = G[name + ".features"], G[name + ".edge_features"]
    ef, ee = out_err(dl.features.cpu().numpy(), wf), out_err(dl.edge_features.cpu().numpy(), we)
    print(name, "node %.3e edge %.3e" % (ef, ee))
    assert ef <= 1e-6 and ee <= 1e-6
    sc = clf.features.scaling
    if clf.regularization.cell_type is not None and "sum" not in sc and "edge" not in sc:      # column 0 is only cast
        assert torch.equal(dl.features[:, 0].cpu(), torch.from_numpy(wf[:, 0]))
    if clf.regularization.edge_type is not None and "sum" not in sc:
        assert torch.equal(dl.edge_features[:, 0].cpu(), torch.from_numpy(we[:, 0]))
    n_node = wf.shape[1] - bool(clf.regularization.cell_type)
    assert dl.getInfo() == wf.shape[0] and clf.temp.num_node_features == n_node
    assert clf.temp.num_edge_features == we.shape[1] - bool(clf.regularization.edge_type)


# ---- 2. ops.scale_features against the model ---------------------------------------------------------------------------------------
def column(rng, j, n):
    k = j % 7
    if k == 0:
        return rng.lognormal(0, 2, n)
    if k == 1:
        return rng.poisson(3, n).astype(np.float64)          # heavy ties across the quantile positions
    if k == 2:
        return np.full(n, 2.5)
    if k == 3:
        return rng.choice(np.array([-1.5, -0.0, 0.0, 0.0, -0.0, 2.0, -3e-5]), n)
    if k == 4:
        return rng.random(n) * 1e-310 * rng.choice([-1.0, 1.0], n)          # denormals
    if k == 5:
        return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-300, 300, n)
    return 1e3 + rng.standard_normal(n) * 1e-3


def frame(n, c, ld, seed, positive=False):
    rng = np.random.default_rng(seed)
    x = np.full((n, ld), 7.0)          # (the padding columns hold finite numbers nobody may read into a result)
    for j in range(c):
        x[:, j] = column(rng, (j + n) if not positive else (j % 2), n)
    if positive:
        x[:, :c] += 0.25
    return x


def run(xd, c, c_first, kind, **kw):
    from dgnn_amd import ops
    out, stats = ops.scale_features(xd[:, :c], c_first, kind, return_stats=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats.cpu().numpy()


NS = [1, 2, 3, 4, 5, 255, 256, 257, 70001]          # 70 001: more rows than the reduce grid's 512 blocks x 64
CS = [1, 20, 29, 65]


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_scalers_match_model(n, c):
    ld = c + 3
    x = frame(n, c, ld, 1000 * c + n)
    xd = torch.from_numpy(x).to(DEV)
    for c_first in (0, 1):
        for kind in M.KINDS:
            for rg in ((0, 1), (-1, 1)) if kind == "minmax" else ((0, 1),):
                want, wstats = M.scale_frame(x[:, :c], c_first, kind, feature_range=rg)
                got, stats = run(xd, c, c_first, kind, feature_range=rg)
                tag = "n %d c %d c_first %d %s %s" % (n, c, c_first, kind, rg)
                if kind == "standard":
                    e0, e1 = stat_err(stats[0], wstats[0], np.abs(wstats[0])), stat_err(stats[1], wstats[1], np.abs(wstats[1]))
                    print(tag, "mean %.3e scale %.3e" % (e0, e1))
                    assert e0 <= 1e-12 and e1 <= 1e-12, tag
                else:          # selected values (or 0 / 1): torch.equal on fp64
                    assert torch.equal(torch.from_numpy(stats), torch.from_numpy(wstats)), tag
                e = out_err(got, want)
                print(tag, "out %.3e" % e)
                assert e <= 1e-6, tag
                if c_first and kind != "none":
                    with np.errstate(over="ignore"):
                        assert np.array_equal(got[:, 0], x[:, 0].astype(np.float32)), tag          # below c_first: the cast alone


# ---- 3. the pre-steps, each alone and chained ------------------------------------------------------------------------------------
def pre_cases(c):
    return {
        "sum": dict(sum_cols=(0, c)),
        "sum1": dict(sum_cols=(1, c)),
        "div": dict(div_col=min(2, c - 1), div_cols=(1, c)),
        "scalar": dict(div_scalar=1.7320508, scalar_cols=(0, c)),
        "sum+div": dict(sum_cols=(1, c), div_col=min(2, c - 1), div_cols=(1, c)),
        "sum+div+scalar": dict(sum_cols=(0, c), div_col=min(2, c - 1), div_cols=(1, c), div_scalar=0.37, scalar_cols=(0, c)),
    }


@pytest.mark.parametrize("n,c", [(5, 20), (257, 29), (70001, 20), (4099, 65)])
def test_pre_steps_match_model(n, c):
    x = frame(n, c, c + 1, 77 * n + c, positive=True)
    xd = torch.from_numpy(x).to(DEV)
    for name, pre in pre_cases(c).items():
        for kind, c_first in (("none", 0), ("standard", 1), ("minmax", 0), ("robust", 1)):
            want, wstats = M.scale_frame(x[:, :c], c_first, kind, feature_range=(-1, 1), **pre)
            got, stats = run(xd, c, c_first, kind, feature_range=(-1, 1), **pre)
            tag = "n %d c %d %s %s" % (n, c, name, kind)
            e0 = stat_err(stats[0], wstats[0], np.abs(wstats[0]))
            e1 = stat_err(stats[1], wstats[1], np.abs(wstats[1]))
            e = out_err(got, want)
            print(tag, "sub %.3e div %.3e out %.3e" % (e0, e1, e))
            assert e0 <= 1e-12 and e1 <= 1e-12 and e <= 1e-6, tag


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------
def test_reruns_are_bit_identical():
    n, c = 70001, 29
    xd = torch.from_numpy(frame(n, c, c + 3, 5)).to(DEV)
    pre = dict(sum_cols=(1, c), div_col=2, div_cols=(1, c))
    for kind in ("standard", "minmax", "robust"):
        for kw in ({}, pre):
            a, sa = run(xd, c, 1, kind, **kw)
            b, sb = run(xd, c, 1, kind, **kw)
            assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(sa.view(np.int64), sb.view(np.int64)), kind


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------
def test_minmax_scene_feeds_inference():
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import SurfaceNet
    from dgnn_amd.processing.data import dataLoader
    dl = dataLoader(clf_for(dict(CONFIGS)["n01"]), verbosity=0)
    dl.run(SCENE_D)
    net = SurfaceNet(reconbench_pretrained(device=DEV))
    net.load_state_dict(kf96_state_dict())
    net = net.to(DEV).eval()
    logits = net.inference_layer(Config(x=dl.features, edge_attr=dl.edge_features, edge_index=dl.edge_lists))
    with torch.no_grad():
        want = oracle_static().inference_layer(Config(x=torch.from_numpy(G["n01.features"]), edge_attr=torch.from_numpy(G["n01.edge_features"]),
                                                      edge_index=torch.from_numpy(gold("ingest_small.npz")["edge_lists"])))
    assert (logits.cpu() - want).abs().max().item() <= TOL_LOGIT * max(1.0, want.abs().max().item())
