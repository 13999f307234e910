#!/usr/bin/env python
"""Times ops.voxel_subsample, ops.min_distance_thin and subsample_scan on scan_mesh scans of a sphere and writes the tables of
profiles/scan_subsample.md.

Whole calls, synchronisations included (validation, the sort, the bins, every round's read-back), one warm-up, the median of 3 (one timed run
for a call of more than 2 s).  Per scan size: the voxel grid at edges giving about 2, 8 and 32 points per voxel against numpy's unique on the
same keys; the thinning at 1, 2 and 4 mean spacings with its rounds and candidates per point, a sweep of the resolution about the default, the
all-pairs kernel where it is affordable, and scipy's cKDTree.query_pairs with the greedy walk on the host when scipy imports; then a scene from
the whole scan against a scene from the subsampled one, stage by stage.

    python tools/bench_scan_subsample.py --out profiles/scan_subsample_measured.md
"""
import argparse
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

from dgnn_amd import ops  # noqa: E402
from bench_knn import timed  # noqa: E402
from bench_mesh_distance import uv_sphere  # noqa: E402

DEV = "cuda:0"


def host_voxel_unique(p, h):
    c = np.floor(p / h).astype(np.int64) + (1 << 20)
    return np.unique((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], return_inverse=True)


def host_greedy(p, r, seed):
    """cKDTree.query_pairs + the sequential walk in the hashed order -> (keep, seconds of the pairs, seconds of the walk)"""
    from scipy.spatial import cKDTree
    import scan_subsample_model as sm
    t0 = time.perf_counter()
    pairs = cKDTree(p).query_pairs(r * (1.0 + 2.0 ** -40), output_type="ndarray")          # a superset; the exact test follows
    d = p[pairs[:, 0]] - p[pairs[:, 1]]
    pairs = pairs[(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] < np.float64(r) * np.float64(r)]
    t1 = time.perf_counter()
    n = len(p)
    base = np.uint64(sm.mix(seed + sm.GOLDEN))
    with np.errstate(over="ignore"):
        z = base + np.arange(n, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    rank = np.empty(n, np.int64)
    rank[np.lexsort((np.arange(n), z))] = np.arange(n)
    later = np.where(rank[pairs[:, 0]] > rank[pairs[:, 1]], pairs[:, 0], pairs[:, 1])
    earlier = pairs[:, 0] + pairs[:, 1] - later
    order = np.argsort(rank[later], kind="stable")          # the pairs grouped by their later point, in the order of the walk
    later_rank, earlier = rank[later][order], earlier[order]
    start = np.searchsorted(later_rank, np.arange(n + 1))
    by_rank = np.argsort(rank)
    keep = np.ones(n, bool)
    for k in range(n):
        keep[by_rank[k]] = not keep[earlier[start[k]:start[k + 1]]].any()
    return keep, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[150000, 1000000])
    ap.add_argument("--per-voxel", type=float, nargs="+", default=[2, 8, 32])
    ap.add_argument("--spacings", type=float, nargs="+", default=[1, 2, 4], help="thinning radii in mean spacings")
    ap.add_argument("--sweep", type=float, nargs="*", default=[0.25, 0.5, 0.7, 1.4, 2.0], help="resolutions swept, as multiples of the default")
    ap.add_argument("--all-pairs-limit", type=float, default=3e10, help="no all-pairs run above this many (point, point) pairs")
    ap.add_argument("--host-limit", type=int, default=200000, help="no host greedy above this many points")
    ap.add_argument("--scene-size", type=int, default=150000, help="the scan size of the scene table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scan_subsample: no GPU (a measurement does not fall back)")
    from dgnn_amd.processing.scan_mesh import scan_mesh
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    v, f = uv_sphere(100, 100)
    scans = {}
    for size in args.sizes:
        scan = scans[size] = scan_mesh(v, f, points=size, cameras=10, noise=0.002, seed=1, device=DEV)
        host = scan["points"]
        p = torch.from_numpy(host).to(DEV)
        n = p.size(0)
        spacing = math.sqrt(4.0 * math.pi / n)          # the unit sphere's area per point, as an edge
        extent = float((host.max(axis=0) - host.min(axis=0)).max())
        say("")
        say("%d points, longest extent %.3f, mean spacing sqrt(4 pi / n) = %.5f" % (n, extent, spacing))
        say("")
        say("| points | voxel edge | voxels | points / voxel | largest voxel | ops.voxel_subsample ms | numpy floor + unique (return_inverse) on the host ms |")
        say("|---|---|---|---|---|---|---|")
        for per in args.per_voxel:
            h = spacing * math.sqrt(per)
            ms, out = timed(lambda: ops.voxel_subsample(p, h))
            t0 = time.perf_counter()
            uniq, inv = host_voxel_unique(host, h)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert len(uniq) == out["m"]
            say("| %d | %.5f (%.1f spacings) | %d | %.2f | %d | %.2f | %.0f |" % (n, h, h / spacing, out["m"], n / out["m"], int(out["count"].max()), ms, host_ms))
        say("")
        say("| points | radius | what | grid_resolution | ms | kept | rounds | candidates / point |")
        say("|---|---|---|---|---|---|---|---|")
        for mult in args.spacings:
            r = mult * spacing
            R0 = ops.default_thin_resolution(extent, r)

            def row(what, R, label):
                ms, (keep, st) = timed(lambda: ops.min_distance_thin(p, r, grid_resolution=R, return_stats=True))
                say("| %d | %.5f (%g spacings) | %s | %s | %.2f | %d | %d | %.1f |" % (n, r, mult, what, label, ms, st["n_kept"], st["rounds"], st["candidates"] / n))
                return keep

            want = row("grid", R0, "%d (default)" % R0)
            for factor in args.sweep:
                R = max(1, min(1024, int(round(R0 * factor))))
                if R != R0 and not torch.equal(row("grid", R, "%d (%.2f x)" % (R, factor)), want):
                    say("| %d | | resolution %d DIFFERS from the default | | | | | |" % (n, R))
            if mult == 2 and float(n) * n <= args.all_pairs_limit:
                say("| %d | | all pairs == default in every byte: %s | | | | | |" % (n, torch.equal(row("all pairs", 0, "0"), want)))
            if mult == 2 and n <= args.host_limit:
                try:
                    keep, t_pairs, t_walk = host_greedy(host, r, 0)
                    say("| %d | %.5f (%g spacings) | scipy cKDTree.query_pairs %.0f ms + the greedy walk in numpy / Python %.0f ms, one thread: == the device: %s "
                        "| | %.0f | %d | | |" % (n, r, mult, t_pairs * 1e3, t_walk * 1e3, bool(np.array_equal(keep, want.cpu().numpy())), (t_pairs + t_walk) * 1e3,
                                                 keep.sum()))
                except ImportError:
                    say("| %d | | scipy does not import: no host comparison | | | | | |" % n)

    from dgnn_amd.processing.scan_scene import clean_scan, subsample_scan
    from dgnn_amd.processing.scene_features import build_scene_features
    from dgnn_amd.processing.triangulate import triangulate_scan
    size = args.scene_size
    scan = scans.get(size) or scan_mesh(v, f, points=size, cameras=10, noise=0.002, seed=1, device=DEV)
    n = len(scan["points"])
    spacing = math.sqrt(4.0 * math.pi / n)

    def scene(points, sensors, label):
        with tempfile.TemporaryDirectory() as tmp:
            base = os.path.join(tmp, "0")
            ms_c, cleaned = timed(lambda: clean_scan(points, sensors, device=DEV), repeats=1)
            ms_t, tri = timed(lambda: triangulate_scan(cleaned["points"], out_base=base, device=DEV), repeats=1)
            ms_f, _ = timed(lambda: build_scene_features(tri["mdata"], tri["infinite"], cleaned["points"], cleaned["sensor_position"], out_base=base, device=DEV),
                            repeats=1)
        say("| %s | %d | %d | %.1f | %.1f | %.1f |" % (label, len(cleaned["kept"]), len(tri["infinite"]), ms_c, ms_t, ms_f))

    say("")
    say("| scan of %d points | points triangulated | cells | clean_scan ms | triangulate_scan ms | build_scene_features ms |" % n)
    say("|---|---|---|---|---|---|")
    scene(scan["points"], scan["sensor_position"], "as it is")
    for label, kw in (("voxel_size = 2 spacings", dict(voxel_size=2.0 * spacing)), ("min_distance = 2 spacings", dict(min_distance=2.0 * spacing)),
                      ("voxel_size = 2 spacings, then min_distance = 2 spacings", dict(voxel_size=2.0 * spacing, min_distance=2.0 * spacing)),
                      ("voxel_size = 4 spacings, then min_distance = 4 spacings", dict(voxel_size=4.0 * spacing, min_distance=4.0 * spacing))):
        ms, sub = timed(lambda: subsample_scan(scan["points"], scan["sensor_position"], device=DEV, **kw))
        scene(sub["points"], sub["sensor_position"], "subsample_scan(%s): %.1f ms, host copies included" % (label, ms))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
