#!/usr/bin/env python
"""Times ops.point_mesh_distance on sphere meshes and writes the table of profiles/mesh_distance.md.

Whole calls, synchronisations included (the planning call, the grid build, the search), one warm-up, the median of 3 (one timed run for a
call of more than 2 s).  Per case: the time, the shells and face evaluations per query, against the all-pairs kernel (grid_resolution = 0)
and ops.nearest_neighbor on as many samples of the same mesh; a sweep of the resolution about default_grid_resolution(F); the same queries
sorted by their start cell.

    python tools/bench_mesh_distance.py --out profiles/mesh_distance_measured.md
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from dgnn_amd import ops  # noqa: E402

DEV = "cuda:0"


def uv_sphere(n_lat, n_lon):
    """a closed unit sphere: 2 n_lon (n_lat - 1) faces"""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon))], -1).reshape(-1, 3)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]])
    idx = 1 + np.arange((n_lat - 1) * n_lon).reshape(n_lat - 1, n_lon)
    nxt = np.roll(idx, -1, axis=1)
    quads = np.stack([idx[:-1], idx[1:], nxt[1:], idx[:-1], nxt[1:], nxt[:-1]], -1).reshape(-1, 3)
    top = np.stack([np.zeros(n_lon, np.int64), idx[0], nxt[0]], -1)
    bot = np.stack([np.full(n_lon, len(v) - 1), nxt[-1], idx[-1]], -1)
    return v, np.concatenate([top, quads, bot]).astype(np.int32)


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


def same_bytes(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:4], b[:4]))


def sort_by_cell(p, R):
    lo, hi = p.min(0).values, p.max(0).values
    c = ((p - lo) / (hi - lo).max() * R).long().clamp_(0, R - 1)
    return p[torch.argsort((c[:, 0] * R + c[:, 1]) * R + c[:, 2])].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[224, 708], help="n_lat = n_lon of the spheres")
    ap.add_argument("--all-pairs-limit", type=float, default=2e11, help="no all-pairs run above this many (point, face) pairs")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_distance: no GPU (a measurement does not fall back)")
    n = args.queries
    lines = ["| faces | queries | grid_resolution | ms | shells / query | max shells | faces evaluated / query | entries |", "|---|---|---|---|---|---|---|---|"]
    for size in args.sizes:
        v, f = uv_sphere(size, size)
        vd, fd = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
        near = ops.sample_interface(vd * 1.01, fd, None, n, seed=1)[0].double()
        far = ops.box_points(n, 2.2, seed=2, device=DEV)
        R0 = ops.default_grid_resolution(len(f))

        def row(kind, q, R, label=None, repeats=3):
            ms, out = timed(lambda: ops.point_mesh_distance(vd, fd, q, grid_resolution=R, return_stats=True), repeats)
            st = out[4]
            lines.append("| %d | %s | %s | %.2f | %.2f | %d | %.1f | %d |" % (len(f), kind, label or R, ms, st["shells"] / n, st["max_shells"],
                                                                          st["faces_evaluated"] / n, st["entries"]))
            print(lines[-1], flush=True)
            return out, ms

        want, _ = row("near", near, R0, "%d (default)" % R0)
        for R in sorted({max(1, R0 // 4), max(1, R0 // 2), min(1024, R0 * 2), min(1024, R0 * 4)} - {R0}):
            row("near", near, R)
        row("near, sorted by cell", sort_by_cell(near, R0), R0, "%d (default)" % R0)
        want_far, ms_far = row("far", far, R0, "%d (default)" % R0)
        got, _ = row("far", far, max(1, R0 // 4))
        lines.append("| %d | far | the two resolutions agree in every byte: %s | | | | | |" % (len(f), same_bytes(got, want_far)))
        print(lines[-1], flush=True)
        if ms_far < 5000.0:          # (a call of many seconds is not repeated in another order)
            row("far, sorted by cell", sort_by_cell(far, R0), R0, "%d (default)" % R0)
        if float(n) * len(f) <= args.all_pairs_limit:
            for kind, q, ref in (("near", near, want), ("far", far, want_far)):
                got, _ = row(kind, q, 0, "0 (all pairs)", repeats=1)
                lines.append("| %d | %s | all pairs == default in every byte: %s | | | | | |" % (len(f), kind, same_bytes(got, ref)))
                print(lines[-1], flush=True)
        samples = ops.sample_interface(vd, fd, None, n, seed=3)[0]
        ms, _ = timed(lambda: ops.nearest_neighbor(samples, near))
        lines.append("| %d | near | nearest_neighbor on %d samples | %.2f | | | | |" % (len(f), n, ms))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
