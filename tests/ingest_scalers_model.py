"""TEST INFRASTRUCTURE ONLY.  numpy fp64 restatement of the reference's feature scaling (processing/data.py:444-506
followed by the float32 cast of :512-519): the pre-steps, the three sklearn scalers and the decision tree that picks
them from the config.  It needs neither pandas nor sklearn; tests/golden/ingest_scalers.npz (the reference's own
dataLoader on tests/golden/scene_small, tests/golden/make_golden_scalers.py) pins it.

Pre-steps, in the reference's order, every one in fp64 with the operations pandas performs:
  sum     x*1000/colsum            over sum_cols = (c0, c1)
  div     x/(x[:, div_col]+1e-4)   over div_cols = (c0, c1); the divisor is the column after `sum`, before `div`
  scalar  x/div_scalar             over scalar_cols = (c0, c1)
Scalers (sklearn 1.7 semantics), fitted on the pre-transformed columns [c_first:]:
  standard  mean, sqrt(population variance), scale < 10 eps -> 1;            (x - mean)/scale
            also scale 1 where var <= n eps var + (n mean eps)^2: sklearn's _is_constant_feature, which keeps a column that a pre-step
            made constant-but-inexact (2*1000/490) at ~0 instead of +-1
  minmax    rg = max - min, rg < 10 eps -> 1; scale = (hi-lo)/rg;            x*scale + (lo - min*scale)
  robust    centre = median, scale = q75 - q25, scale < 10 eps -> 1;         (x - centre)/scale
            quantiles by numpy's linear rule (quantile()); the median of an even count is the mean of the two
            middle values, as numpy's median (which sklearn calls) takes it
  none      cast only
stats [2, C]: what was subtracted and what was divided by (minmax: data_min and the zero-handled data_range);
columns below c_first hold 0 and 1.
"""
import sys

import numpy as np

EPS = np.finfo(np.float64).eps
EPS10 = 10 * EPS
KINDS = ("none", "standard", "minmax", "robust")


def quantile(s: np.ndarray, p: float) -> np.ndarray:
    """numpy's method='linear' on the sorted columns `s` [n, C]"""
    n = s.shape[0]
    h = (n - 1) * p
    lo = int(np.floor(h))
    hi = min(lo + 1, n - 1)
    t = h - lo
    d = s[hi] - s[lo]
    return s[lo] + d * t if t < 0.5 else s[hi] - d * (1 - t)


def median(s: np.ndarray) -> np.ndarray:
    n = s.shape[0]
    return s[n // 2].copy() if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0


def pre_steps(x64, sum_cols=None, div_col=None, div_cols=None, div_scalar=None, scalar_cols=None) -> np.ndarray:
    x = np.array(x64, np.float64, copy=True)
    if sum_cols is not None:
        a, b = sum_cols
        x[:, a:b] = x[:, a:b] * 1000 / x[:, a:b].sum(axis=0)
    if div_cols is not None:
        a, b = div_cols
        x[:, a:b] = x[:, a:b] / (x[:, div_col] + 0.0001)[:, None]
    if scalar_cols is not None:
        a, b = scalar_cols
        x[:, a:b] = x[:, a:b] / div_scalar
    return x


def scale_frame(x64, c_first, kind, feature_range=(0, 1), **pre):
    """-> (float32 [n, C], stats float64 [2, C])"""
    assert kind in KINDS
    x = pre_steps(x64, **pre)
    n, c = x.shape
    stats = np.stack([np.zeros(c), np.ones(c)])
    body = x[:, c_first:]
    if kind == "standard":
        mean = body.mean(axis=0)
        with np.errstate(over="ignore", invalid="ignore"):
            var = ((body - mean) ** 2).mean(axis=0)
            scale = np.sqrt(var)
            scale[(var <= n * EPS * var + (n * mean * EPS) ** 2) | (scale < EPS10)] = 1.0
        x[:, c_first:] = (body - mean) / scale
        stats[0, c_first:], stats[1, c_first:] = mean, scale
    elif kind == "minmax":
        lo, hi = float(feature_range[0]), float(feature_range[1])
        mn = body.min(axis=0) + 0.0            # (-0.0 -> +0.0: the two are one value)
        rg = body.max(axis=0) - mn
        rg[rg < EPS10] = 1.0
        sc = (hi - lo) / rg
        x[:, c_first:] = body * sc + (lo - mn * sc)
        stats[0, c_first:], stats[1, c_first:] = mn, rg
    elif kind == "robust":
        s = np.sort(body, axis=0)
        centre = median(s)
        scale = quantile(s, 0.75) - quantile(s, 0.25)
        scale[scale < EPS10] = 1.0
        with np.errstate(over="ignore"):
            x[:, c_first:] = (body - centre) / scale
        stats[0, c_first:], stats[1, c_first:] = centre, scale
    with np.errstate(over="ignore"):
        return x.astype(np.float32), stats


def plan(scaling, node_norm, edge_norm, cell_type, edge_type, node_names, edge_names, n_node_cols, n_edge_cols, mean_edge,
         normalization_range=None, read_edge_features=True):
    """The reference's decision tree (:446-506) -> (node kwargs, edge kwargs or None) for scale_frame.  `in` is applied to whatever the
    config holds, string or list, as the reference does."""
    node = dict(c_first=0, kind="none")
    edge = dict(c_first=0, kind="none")
    if not scaling:                                            # :108  no scaling key: cast only
        return node, (edge if read_edge_features else None)
    if "sum" in scaling:                                       # :446-452
        node["sum_cols"] = (1 if node_norm else 0, n_node_cols)
        edge["sum_cols"] = (0, n_edge_cols)
    if "vol" in scaling:                                       # :454-459
        print("scaling 'vol' is not supported (the reference cannot run it either)")
        sys.exit(1)
    if node_norm is not None:                                  # :461-465
        if cell_type is None:
            raise KeyError(None)
        node["div_col"], node["div_cols"] = node_names.index(cell_type), (1, n_node_cols)
    if "edge" in scaling:                                      # :467-468
        node["div_scalar"], node["scalar_cols"] = mean_edge, (0, n_node_cols)
    if "s" in scaling:                                         # :471-483
        kind = "standard"
    elif "n" in scaling:
        kind = "minmax"
        node["feature_range"] = edge["feature_range"] = tuple(normalization_range)          # :474  (None here: the reference's KeyError)
    elif "r" in scaling:
        kind = "robust"
    elif "sum" not in scaling:
        raise AttributeError("feature_scaling")
    else:
        return node, (edge if read_edge_features else None)    # the edge frame got the sum step only
    node["kind"], node["c_first"] = kind, (1 if cell_type is not None else 0)          # :485-491
    if not read_edge_features:
        return node, None
    if edge_norm is not None:                                  # :495-499
        if edge_type is None:
            raise KeyError(None)
        edge["div_col"], edge["div_cols"] = edge_names.index(edge_type), (1, n_edge_cols)
    edge["kind"], edge["c_first"] = kind, (1 if edge_type is not None else 0)          # :501-506
    return node, edge
