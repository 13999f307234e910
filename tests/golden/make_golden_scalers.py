#!/usr/bin/env python3
"""Generates tests/golden/ingest_scalers.npz by RUNNING THE REFERENCE's own dataLoader on tests/golden/scene_small
with every feature-scaling route of its standardizeFeatures (processing/data.py:444-506).

Run in the authoring container only (needs the reference tree, pandas and sklearn, like make_golden.py):

    python tests/golden/make_golden_scalers.py

The scene is the one make_golden.py's ingest fixture wrote; it is read, never rewritten.  Per config the file holds
``<name>.features`` and ``<name>.edge_features`` (fp32, as the reference's toTorch leaves them); ``configs`` is the
JSON list of the overrides each name stands for (data only; no reference source is copied).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

# name -> overrides of configs/pretrained/reconbench.yaml ("section.key": value)
CONFIGS = [
    ("n01", {"features.scaling": "n", "features.normalization_range": [0, 1]}),
    ("n11", {"features.scaling": "n", "features.normalization_range": [-1, 1]}),
    ("r", {"features.scaling": "r"}),
    ("sum_str", {"features.scaling": "sum"}),
    ("sum_list", {"features.scaling": ["sum"]}),
    ("sum_n", {"features.scaling": ["sum", "n"]}),
    ("edge_s", {"features.scaling": ["edge", "s"]}),
    ("s_nodenorm", {"features.scaling": "s", "features.node_normalization_feature": 1}),
    ("s_edgenorm", {"features.scaling": "s", "features.edge_normalization_feature": 1, "regularization.edge_type": "area"}),
    ("r_edgetype", {"features.scaling": "r", "regularization.edge_type": "area"}),
    ("n_nocell", {"features.scaling": "n", "regularization.cell_type": None}),
]


def apply(clf, overrides):
    for k, v in overrides.items():
        sec, key = k.split(".")
        clf[sec][key] = v
    return clf


def main():
    sys.path.insert(0, mg.REF)
    from processing.data import dataLoader
    root = os.path.join(HERE, "scene_small")
    out = {"configs": np.array(json.dumps(CONFIGS))}
    for name, ov in CONFIGS:
        clf = apply(mg.static_clf(), ov)
        clf.inference.has_label = 1
        dl = dataLoader(clf, verbosity=0)
        dl.run(dict(path=root, filename="0", category="", id="", scan_conf="", gtfile="gt/0", ioufile=""))
        out[name + ".features"] = dl.features.numpy()
        out[name + ".edge_features"] = dl.edge_features.numpy()
        print(name, tuple(dl.features.shape), tuple(dl.edge_features.shape), "max |x| %.4g / %.4g" % (
            np.abs(out[name + ".features"]).max(), np.abs(out[name + ".edge_features"]).max()))
    path = os.path.join(HERE, "ingest_scalers.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
