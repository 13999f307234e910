#!/usr/bin/env python3
"""Generates tests/golden/ignatius_scene_features*.npz from the reference's DATA files of Ignatius scene 99 (no reference code runs).

Run in the authoring container only (needs the reference checkout, REF below):

    python tests/golden/make_golden_scene_features.py

The fixture holds what tests/test_scene_features_cpu.py and tests/test_gpu_scene_features.py need beside ignatius_3dt.npz (vertices,
tetrahedra, infinite) and static_f4_ignatius_full.npz (adj_dst):

* `points`, `sensor_position` of scan/99.npz;
* `facets`, `nfacets` of gt/99_3dt.npz;
* `radius`, `vol`, `longest_edge`, `shortest_edge` of gt/99_cgeom.npz;
* the non-`last` columns of gt/99_cbvf.npz and gt/99_fbvf.npz, stored sparsely: `<group>_rows` = the rows where any column of the group
  (cb / fb x inside / outside) is non-zero, `<column>` = the column at those rows; `cb_rows_total`, `fb_rows_total` = the row counts;
  `vf_keys_cb`, `vf_keys_fb` = the files' twelve keys in file order (the `last` columns hold 0 everywhere, which is checked here).

The cell geometry alone is 2 MB of fp64 mantissas that no compressor shortens, and no committed file may pass 1 MiB: the arrays are
packed, in the order above, into ignatius_scene_features.npz, ignatius_scene_features_2.npz, ... of at most PART_LIMIT bytes each;
scene_features_model.load_fixture reads them back as one dict.
"""
from __future__ import annotations

import glob
import io
import os
import sys

import numpy as np

REF = "/root/reference/data/Ignatius"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import scene_features_model as sf  # noqa: E402

STEM = sf.FIXTURE_STEM
PART_LIMIT = 960 * 1024


def _size(arrays):
    b = io.BytesIO()
    np.savez_compressed(b, **arrays)
    return len(b.getvalue())


def main():
    m = np.load(os.path.join(REF, "gt", "99_3dt.npz"))
    scan = np.load(os.path.join(REF, "scan", "99.npz"))
    cgeom = np.load(os.path.join(REF, "gt", "99_cgeom.npz"))
    out = {"points": scan["points"], "sensor_position": scan["sensor_position"], "facets": m["facets"], "nfacets": m["nfacets"]}
    for k in ("radius", "vol", "longest_edge", "shortest_edge"):
        out[k] = cgeom[k]
    assert list(cgeom.files) == ["radius", "vol", "longest_edge", "shortest_edge"]
    for pre, name in (("cb", "99_cbvf.npz"), ("fb", "99_fbvf.npz")):
        z = np.load(os.path.join(REF, "gt", name))
        out["vf_keys_" + pre] = np.array(z.files)
        out[pre + "_rows_total"] = np.int64(len(z[z.files[0]]))
        for k in z.files:
            assert z[k].dtype == np.float64
            if "_last_" in k:
                assert not z[k].any(), k
        for side in ("inside", "outside"):
            keys = [k for k in z.files if "_%s_" % side in k]
            rows = np.nonzero(np.any([z[k] != 0 for k in keys], axis=0))[0].astype(np.int32)
            out["%s_%s_rows" % (pre, side)] = rows
            for k in keys:
                out[k] = z[k][rows]
    for old in glob.glob(os.path.join(HERE, STEM + "*.npz")):
        os.remove(old)
    parts, cur = [], {}
    for k, a in out.items():
        if cur and _size({**cur, k: a}) > PART_LIMIT:
            parts.append(cur)
            cur = {}
        cur[k] = a
    parts.append(cur)
    for i, part in enumerate(parts):
        path = os.path.join(HERE, STEM + ("" if i == 0 else "_%d" % (i + 1)) + ".npz")
        np.savez_compressed(path, **part)
        print("wrote %s (%d bytes): %s" % (path, os.path.getsize(path), ", ".join(part)))
        assert os.path.getsize(path) < 1024 * 1024
    back = sf.load_fixture(HERE)
    assert all(np.array_equal(back[k], out[k]) for k in out) and len(back) == len(out)


if __name__ == "__main__":
    main()
