"""Times ops.ray_first_hit, the hot part of the virtual scanner (dgnn_amd/processing/scan_mesh.py), over a sweep of grid resolutions R and
writes profiles/scan_mesh.md.

Two closed meshes, the scanner's own rays (10 cameras at distance 2, aims from ops.sample_interface):
  small  the interface of the seeded scipy-Delaunay sphere scene of the other mesh tools (tests/mesh_metrics_model.py: uniform points in
         the unit cube, cells labelled by a sphere), about 1e4 faces at the default 175 000 points; 12 000 rays; R = 1 is in its sweep;
  large  about 1e6 faces, 1 000 000 rays.  A Delaunay interface of that size would need some 2e8 points, so the large mesh is the
         latitude / longitude sphere of tools/bench_mesh_contains.py (long thin faces towards the poles: not a friendly mesh).
Every timing is the host clock around one whole Python call that ends in a device synchronise (plan call, validation, grid build, the
walk, four status reads), after one warm-up per configuration; the configurations ALTERNATE inside every round, and median / min / max over
the rounds are reported.  Every timed result is checked against the all-pairs numpy model (tests/ray_cast_model.py) on a subsample, and all
resolutions against one another on every ray.  The CPU line is the model's filter-only path on the same host: a numpy all-pairs loop, not a
tuned CPU ray caster, so it is context and not a speed-up claim.

    python tools/bench_scan_mesh.py [--rounds 5] [--out profiles/scan_mesh.md]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mesh_metrics_model as mm  # noqa: E402
import ray_cast_model as rc  # noqa: E402
from bench_mesh_contains import uv_sphere  # noqa: E402
from dgnn_amd import ops  # noqa: E402
from dgnn_amd.processing import scan_mesh as sm  # noqa: E402


def delaunay_interface(n_points, seed=0):
    scene = mm.random_scene(n_points, seed)
    tri = scene["facets"][mm.interface_ids(mm.sphere_labels(scene), scene["nfacets"])].astype(np.int64)
    kept, inv = np.unique(tri, return_inverse=True)
    return scene["vertices"][kept], inv.reshape(-1, 3).astype(np.int32)


def scanner_rays(v, f, n, cameras=10, seed=0):
    """the rays scan_mesh casts -> (origins, aims) fp64 on the GPU"""
    s1, s2 = (int(x) for x in sm.mm_hash(seed, np.arange(1, 3, dtype=np.uint64)))
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    aims, _ = ops.sample_interface(vd, fd, None, n, seed=s1)
    cams = torch.from_numpy(sm.camera_positions(v, f, cameras, 2.0, seed)).cuda()
    ids = torch.from_numpy((sm.mm_hash(s2, np.arange(1, n + 1, dtype=np.uint64)) % np.uint64(cameras)).astype(np.int64)).cuda()
    return vd, fd, cams[ids].contiguous(), aims.to(torch.float64)


def sweep(name, v, f, n_rays, resolutions, rounds, model_rays, cpu_rays):
    vd, fd, o, g = scanner_rays(v, f, n_rays)
    default = ops.default_grid_resolution(len(f))
    configs = list(resolutions) + ([default] if default not in resolutions else [])
    times = {R: [] for R in configs}
    results = {}
    for R in configs:          # warm-up of every configuration (code objects, allocator)
        results[R] = ops.ray_first_hit(vd, fd, o, g, grid_resolution=R, return_stats=True)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for R in configs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.ray_first_hit(vd, fd, o, g, grid_resolution=R)
            torch.cuda.synchronize()
            times[R].append(1e3 * (time.perf_counter() - t0))
    first = results[configs[0]]
    same = all(torch.equal(first[0], r[0]) and torch.equal(first[1].view(torch.int64), r[1].view(torch.int64)) and first[3] == r[3] for r in results.values())
    sub = np.linspace(0, n_rays - 1, model_rays).astype(np.int64)
    oh, gh = o.cpu().numpy(), g.cpu().numpy()
    t0 = time.perf_counter()
    want = rc.first_hit(v, f, oh[sub], gh[sub], chunk=max(1, 2 ** 22 // len(f)))
    model_s = time.perf_counter() - t0
    model_equal = bool(np.array_equal(first[0].cpu().numpy()[sub], want[0]) and
                       np.array_equal(first[1].cpu().numpy()[sub].view(np.int64), want[1].view(np.int64)))
    t0 = time.perf_counter()
    rc.filter_only_first_hit(v, f, oh[:cpu_rays], gh[:cpu_rays], chunk=max(1, 2 ** 22 // len(f)))
    cpu_s = time.perf_counter() - t0
    rows = [dict(R=R, entries=None, ms_median=float(np.median(times[R])), ms_min=min(times[R]), ms_max=max(times[R])) for R in configs]
    for row in rows:
        n_entries = sm_entries(vd, fd, row["R"])
        row["entries"] = n_entries
    res = dict(mesh=name, faces=len(f), vertices=len(v), rays=n_rays, rounds=rounds, default_R=default, rows=rows, all_resolutions_equal=bool(same),
               stats=first[3], model_rays=model_rays, model_equal=model_equal, model_s=model_s, cpu_rays=cpu_rays, cpu_s=cpu_s)
    print(json.dumps(res), flush=True)
    return res


def sm_entries(vd, fd, R):
    """the (face, cell) entries of the grid at resolution R (dgnn_ray_first_hit_plan)"""
    import ctypes as C

    from dgnn_amd._lib import check, lib, ptr, stream_ptr
    scratch = torch.empty(int(lib().dgnn_ray_first_hit_scratch_bytes(fd.size(0), R)), dtype=torch.uint8, device=vd.device)
    n = C.c_int64(0)
    check(lib().dgnn_ray_first_hit_plan(ptr(vd), vd.size(0), ptr(fd), fd.size(0), R, C.byref(n), None, ptr(scratch), stream_ptr()), "dgnn_ray_first_hit_plan")
    return int(n.value)


def write_report(path, results, rounds):
    lines = ["# `ops.ray_first_hit`: the virtual scanner's rays over a sweep of grid resolutions", "",
             "Generated by `python tools/bench_scan_mesh.py` on an MI355X (gfx950, other tenants on the host), profiler off.  Each figure is the host",
             "clock around one whole `ops.ray_first_hit` call ending in a device synchronise (plan call, validation, grid build, the walk, the status",
             "reads), after one warm-up per configuration; the configurations alternate inside each of the %d rounds; median / min / max." % rounds,
             "The rays are the scanner's: 10 cameras at distance 2, aims from `ops.sample_interface`.", ""]
    for r in results:
        lines += ["## %s: %d faces, %d rays" % (r["mesh"], r["faces"], r["rays"]), "", "| R | (face, cell) entries | ms median | min | max | Mrays/s at the median |",
                  "|---|---|---|---|---|---|"]
        for row in r["rows"]:
            mark = " (default)" if row["R"] == r["default_R"] else ""
            lines.append("| %d%s | %d | %.3f | %.3f | %.3f | %.2f |" % (row["R"], mark, row["entries"], row["ms_median"], row["ms_min"], row["ms_max"],
                                                                         r["rays"] / row["ms_median"] / 1e3))
        best = min(r["rows"], key=lambda x: x["ms_median"])
        dflt = next(x for x in r["rows"] if x["R"] == r["default_R"])
        lines += ["", "Fastest: R = %d (%.3f ms); the default `ops.default_grid_resolution(%d)` = %d takes %.3f ms, %.0f %% above it." % (
                      best["R"], best["ms_median"], r["faces"], r["default_R"], dflt["ms_median"], 100 * (dflt["ms_median"] / best["ms_median"] - 1)),
                  "All resolutions give the same faces, the same bits of t and the same stats: %s.  Stats: %s." % (r["all_resolutions_equal"], r["stats"]),
                  "Against the all-pairs numpy model on %d rays spread over the set: equal = %s (the model took %.1f s)." % (r["model_rays"], r["model_equal"], r["model_s"]),
                  "CPU line: the model's filter-only all-pairs path on the same host, %d rays in %.2f s = %.0f rays/s.  It is a test oracle in numpy," % (
                      r["cpu_rays"], r["cpu_s"], r["cpu_rays"] / r["cpu_s"]),
                  "not a tuned CPU ray caster: context, not a speed-up figure.", ""]
    lines += ["## The default", "",
              "`ops.default_grid_resolution(n_faces) = clamp(round(sqrt(n_faces) / 2), 1, 256)`: a closed surface of F faces fills about R^2 cells of",
              "the grid, so R ~ sqrt(F) keeps a handful of faces per occupied cell, and the cap bounds the R^3 cell arrays (256^3 cells: 134 MB).",
              "The tables above say how far that rule is from the best R of the sweep on these two meshes: where an R above the cap is faster, it is so",
              "at a million rays and for 8 times the cell arrays (512^3 cells: 1.07 GB, zeroed and scanned in every call), which a call with few rays",
              "would pay without the gain, so the cap stays.  The answer does not depend on R.", "",
              "Not measured: the kernel's own time (a `rocprofv3 --kernel-trace` run), the share of the six stream synchronisations of the two calls,",
              "meshes with very large faces, origins inside the mesh, other ray counts.  No timing is a pass condition of any test.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small-points", type=int, default=175000)
    ap.add_argument("--rings", type=int, default=500)
    ap.add_argument("--small-sweep", type=int, nargs="+", default=[1, 8, 16, 32, 64, 128, 256])
    ap.add_argument("--large-sweep", type=int, nargs="+", default=[32, 64, 128, 256, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_mesh.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scan_mesh needs a GPU")
    results = [sweep("small (Delaunay sphere interface)", *delaunay_interface(a.small_points), 12000, a.small_sweep, a.rounds, 64, 256)]
    v, f = uv_sphere(a.rings)
    results.append(sweep("large (latitude / longitude sphere)", v, f, 1000000, a.large_sweep, a.rounds, 4, 4))
    write_report(a.out, results, a.rounds)


if __name__ == "__main__":
    main()
