#!/usr/bin/env python
"""Times ops.knn and the scan operations on it on scan_mesh scans of a sphere and writes the tables of profiles/knn.md.

Whole calls, synchronisations included (validation, the bins, the search), one warm-up, the median of 3 (one timed run for a call of more
than 2 s).  Per scan size and k: the grid path at the default resolution with its shells and candidates per query; a sweep of the resolution
about the default; the same queries walked in input order (the points passed as separate queries) against the cell order; the all-pairs
kernel; ops.nearest_neighbor on the same points; scipy's cKDTree on the host when scipy imports; then outlier_mask, estimate_normals and
scene_from_scan stage by stage.

    python tools/bench_knn.py --out profiles/knn_measured.md
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from dgnn_amd import ops  # noqa: E402
from bench_mesh_distance import uv_sphere  # noqa: E402

DEV = "cuda:0"


def timed(fn, repeats=3):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    if time.perf_counter() - t0 > 2.0:          # a call of seconds: one timed run after the warm-up
        repeats = 1
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[150000, 1000000])
    ap.add_argument("--ks", type=int, nargs="+", default=[8, 16, 32, 64])
    ap.add_argument("--sweep", type=float, nargs="*", default=[0.25, 0.35, 0.5, 0.7, 1.4, 2.0, 4.0], help="resolutions swept, as multiples of the default")
    ap.add_argument("--all-pairs-limit", type=float, default=3e10, help="no all-pairs run above this many (query, point) pairs")
    ap.add_argument("--stages-size", type=int, default=150000, help="the scan size of the stage-by-stage table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn: no GPU (a measurement does not fall back)")
    from dgnn_amd.processing.scan_mesh import scan_mesh
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    v, f = uv_sphere(100, 100)
    scans = {}
    say("| points | k | what | grid_resolution | ms | shells / query | candidates / query | placed / query |")
    say("|---|---|---|---|---|---|---|---|")
    for size in args.sizes:
        scan = scans[size] = scan_mesh(v, f, points=size, cameras=10, noise=0.002, seed=1, device=DEV)
        p = torch.from_numpy(scan["points"]).to(DEV)
        n = p.size(0)
        R0 = ops.default_knn_resolution(n)

        def row(k, what, R, queries=None, label=None):
            ms, out = timed(lambda: ops.knn(p, k, queries=queries, grid_resolution=R, return_stats=True))
            st = out[2]
            say("| %d | %d | %s | %s | %.2f | %.2f | %.1f | %.1f |" % (n, k, what, label or R, ms, st["shells"] / n, st["candidates"] / n, st["placed"] / n))
            return out

        for k in args.ks:
            want = row(k, "grid, cell order", R0, label="%d (default)" % R0)
            for factor in args.sweep:
                R = max(1, min(1024, int(round(R0 * factor))))
                got = row(k, "grid, cell order", R, label="%d (%.2f x)" % (R, factor))
                if not (torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])):
                    say("| %d | %d | resolution %d DIFFERS from the default | | | | | |" % (n, k, R))
            if k == 16:
                row(k, "grid, input order (the points as separate queries)", R0, queries=p, label="%d (default)" % R0)
                if float(n) * n <= args.all_pairs_limit:
                    got = row(k, "all pairs", 0, label="0")
                    say("| %d | %d | all pairs == default in every byte: %s | | | | | |" % (n, k, torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])))
        ms, _ = timed(lambda: ops.nearest_neighbor(p, p))
        say("| %d | 1 | ops.nearest_neighbor (fp32, the points against themselves) | | %.2f | | | |" % (n, ms))
        try:
            from scipy.spatial import cKDTree
            host = scan["points"]
            for k in (16,):
                t0 = time.perf_counter()
                tree = cKDTree(host)
                tree.query(host, k=k + 1)
                say("| %d | %d | scipy cKDTree build + query on the host, one thread | | %.0f | | | |" % (n, k, (time.perf_counter() - t0) * 1e3))
        except ImportError:
            say("| %d | | scipy does not import: no host comparison | | | | | |" % n)

    from dgnn_amd.processing.scan_scene import clean_scan
    from dgnn_amd.processing.scene_features import build_scene_features
    from dgnn_amd.processing.triangulate import triangulate_scan
    size = args.stages_size
    scan = scans.get(size) or scan_mesh(v, f, points=size, cameras=10, noise=0.002, seed=1, device=DEV)
    noisy = scan_mesh(v, f, points=size, cameras=10, noise=0.002, outliers=0.05, seed=1, device=DEV)
    p = torch.from_numpy(noisy["points"]).to(DEV)
    say("")
    say("| stage on %d points (5 %% outliers) | ms |" % p.size(0))
    say("|---|---|")
    ms, (keep, st) = timed(lambda: ops.outlier_mask(p))
    say("| ops.outlier_mask (k = 16): %d removed | %.2f |" % (st["n_removed"], ms))
    ms, _ = timed(lambda: ops.estimate_normals(p, sensors=torch.from_numpy(noisy["sensor_position"]).to(DEV)))
    say("| ops.estimate_normals (k = 16, sensors) | %.2f |" % ms)
    ms, cleaned = timed(lambda: clean_scan(noisy["points"], noisy["sensor_position"], device=DEV), repeats=1)
    say("| clean_scan (both, host copies included): %d kept | %.2f |" % (len(cleaned["kept"]), ms))
    injected = noisy["hit_face"] < 0
    removed = np.setdiff1d(np.arange(len(injected)), cleaned["kept"])
    say("| of %d injected outliers %d removed; of %d surface points %d removed | |" % (injected.sum(), injected[removed].sum(), (~injected).sum(), (~injected[removed]).sum()))
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "0")
        ms, tri = timed(lambda: triangulate_scan(cleaned["points"], out_base=base, device=DEV), repeats=1)
        say("| triangulate_scan: %d cells | %.2f |" % (len(tri["infinite"]), ms))
        ms, _ = timed(lambda: build_scene_features(tri["mdata"], tri["infinite"], cleaned["points"], cleaned["sensor_position"], out_base=base, device=DEV,
                                                   facet_rays=True, facet_geometry=True), repeats=1)
        say("| build_scene_features (facet_rays, facet_geometry) | %.2f |" % ms)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
