"""Times ops.ray_walk -- every scan ray walked through all the cells it crosses -- on a scanned scene at bench scale (a sphere
mesh scanned with 150 000 rays, triangulated by ops.delaunay) and on the Ignatius fixture: whole calls with their synchronisations, one
warm-up, the median of --reps; then once more with the library's stage timing on (it synchronises at every stage boundary, so the stages
add up to more than the plain call).  Reports rays, records per ray, the longest walk, perturbed / exact_used, the workspace at the default
max_records and the registers of the walk kernel (a compile of csrc/raywalk.hip with the resource remarks, skipped without hipcc).

It also records the classical baseline on a scanned sphere: the agreement of the visibility-vote graph cut (processing.visibility) with the
majority label of build_cell_labels, next to the agreement of labelling every cell outside.  A record, not a threshold.

    python tools/bench_ray_walk.py [--points 150000] [--reps 3] [--out profiles/ray_walk.md]
"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mesh_contains_model as mc  # noqa: E402
import scene_features_model as sf  # noqa: E402
from dgnn_amd import ops  # noqa: E402
from dgnn_amd._lib import lib  # noqa: E402

STAGES = ("checks + start + counting walk", "filling walk", "sort", "fold")


def _time(fn, reps):
    fn()   # warm-up (code objects, allocator)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, 1e3 * float(np.median(times))


def bench(name, v, tets, nbr, rv, s, reps, **depths):
    inc = ops.vertex_incidence(tets, v.size(0))
    call = lambda: ops.ray_walk(v, tets, nbr, rv, s, incidence=inc, **depths)
    out, ms = _time(call, reps)
    stage = (ctypes.c_double * 4)()
    lib().dgnn_ray_walk_timing(1, None)
    call()
    lib().dgnn_ray_walk_timing(0, stage)
    st = out["stats"]
    m = max(ops.WALK_DEFAULT_RECORDS, tets.size(0) + 1)
    row = dict(scene=name, tets=tets.size(0), rays=rv.numel(), depths=depths, ms_median=ms, stage_ms=dict(zip(STAGES, (float(x) for x in stage))),
               records_per_used_ray=st["records"] / max(st["used"], 1), workspace_bytes=int(lib().dgnn_ray_walk_scratch_bytes(rv.numel(), tets.size(0), v.size(0), m)),
               stats=st)
    print(json.dumps(row), flush=True)
    return row


def kernel_resources():
    """VGPRs and scratch of the walk kernels from the compiler's resource remarks"""
    src = os.path.join(ROOT, "dgnn_amd", "csrc", "raywalk.hip")
    try:
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                            "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull], capture_output=True, text=True, timeout=300)
    except (OSError, subprocess.TimeoutExpired):
        return {}
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for key in ("VGPRs", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]"):
            m = re.search(r"\s%s: (\d+)" % key, line)
            if m and name and ("k_walk" in name) and ("6k_walkILb" in name or "k_walk_start" in name):
                short = "k_walk_start" if "k_walk_start" in name else "k_walk<%s>" % ("false" if "ILb0" in name else "true")
                out.setdefault(short, {})[key.split(" ")[0]] = int(m.group(1))
    return out


def baseline(points, seed=1):
    """a scanned sphere: the visibility votes, cut, against the majority label of the sampled ground truth"""
    from dgnn_amd.processing.scan_mesh import scan_mesh
    from dgnn_amd.processing.scene_features import build_cell_labels, build_scene_features
    from dgnn_amd.processing.triangulate import triangulate_scan
    from dgnn_amd.processing.visibility import visibility_logits
    gv, gf = mc.sphere_interface(300)
    scan = scan_mesh(gv, gf, points=points, cameras=10, seed=seed)
    tri = triangulate_scan(scan["points"], seed=seed)
    feat = build_scene_features(tri["mdata"], tri["infinite"], scan["points"], scan["sensor_position"], facet_rays=True)
    lab = build_cell_labels(tri["mdata"], tri["infinite"], gv, gf, n_samples=100, seed=0)
    truth = (lab["outside_perc"] >= 0.5).astype(np.int32)          # 1 = outside, the graph cut's convention
    adj = tri["adjacencies"]
    edges = adj[adj[:, 0] < adj[:, 1]]
    out = {}
    for bw in (0, 1, 4):
        labels, _, _ = ops.binary_graph_cut(visibility_logits(feat, tri["infinite"], 1000.0), edges, 1.0, float(bw))
        out["cut_binary_weight_%d" % bw] = float((labels.cpu().numpy() == truth).mean())
    out.update(all_outside=float((truth == 1).mean()), cells=int(len(truth)), scan_points=int(len(scan["points"])), walk_stats=feat["walk_stats"])
    print(json.dumps(dict(baseline=out)), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_walk.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ray_walk needs a GPU")
    from dgnn_amd.processing.scan_mesh import scan_mesh
    from dgnn_amd.processing.triangulate import triangulate_scan
    rows = []
    gv, gf = mc.sphere_interface(300)
    scan = scan_mesh(gv, gf, points=a.points, cameras=10, noise=0.002, seed=0)
    tri = triangulate_scan(scan["points"], seed=0)
    md = tri["mdata"]
    v, tets = torch.from_numpy(md["vertices"]).cuda(), torch.from_numpy(md["tetrahedra"]).cuda()
    nbr = ops.tet_neighbors(torch.from_numpy(md["facets"]).cuda(), torch.from_numpy(md["nfacets"]).cuda(), tets)
    vid = sf.match_vertices(md["vertices"], scan["points"])
    rv, s = torch.from_numpy(vid).cuda(), torch.from_numpy(scan["sensor_position"]).cuda()
    rows.append(bench("scanned sphere, noise 0.002", v, tets, nbr, rv, s, a.reps, outside_depth=0, inside_depth=1))
    rows.append(bench("scanned sphere, noise 0.002", v, tets, nbr, rv, s, a.reps, outside_depth=0, inside_depth=0))
    fx, g = sf.load_fixture(), np.load(os.path.join(ROOT, "tests", "golden", "ignatius_3dt.npz"))
    v, tets = torch.from_numpy(g["vertices"]).cuda(), torch.from_numpy(g["tetrahedra"]).cuda()
    nbr = ops.tet_neighbors(torch.from_numpy(fx["facets"]).cuda(), torch.from_numpy(fx["nfacets"]).cuda(), tets)
    rv, s = torch.from_numpy(sf.match_vertices(g["vertices"], fx["points"])).cuda(), torch.from_numpy(fx["sensor_position"]).cuda()
    rows.append(bench("ignatius", v, tets, nbr, rv, s, a.reps, outside_depth=0, inside_depth=1))
    rows.append(bench("ignatius", v, tets, nbr, rv, s, a.reps, outside_depth=0, inside_depth=0))
    base = baseline(20000)
    res = kernel_resources()
    with open(a.out, "w") as fh:
        fh.write("# `ops.ray_walk`: every scan ray through all the cells it crosses\n\n")
        fh.write("Written by `tools/bench_ray_walk.py`.  Whole calls with their synchronisations, one warm-up, median of %d; the stage columns come from one\n"
                 "more call with the library's stage timing on, which synchronises at every stage boundary.\n\n" % a.reps)
        fh.write("| scene | tets | rays | depths (out, in) | call (ms) | records / used ray | longest walk | perturbed | exact_used | stuck | capped | "
                 + " | ".join("%s (ms)" % x for x in STAGES) + " | workspace (MiB) |\n|" + "---|" * 16 + "\n")
        for r in rows:
            st = r["stats"]
            fh.write("| %s | %d | %d | %d, %d | %.2f | %.2f | %d | %d | %d | %d | %d | %s | %.1f |\n" % (
                r["scene"], r["tets"], r["rays"], r["depths"]["outside_depth"], r["depths"]["inside_depth"], r["ms_median"], r["records_per_used_ray"],
                st["longest"], st["perturbed"], st["exact_used"], st["stuck"], st["capped"], " | ".join("%.2f" % r["stage_ms"][x] for x in STAGES),
                r["workspace_bytes"] / 2 ** 20))
        fh.write("\nKernel resources (compiler remarks, gfx950):\n\n| kernel | VGPRs | scratch (bytes / lane) | waves / SIMD |\n|---|---|---|---|\n")
        for k, d in sorted(res.items()):
            fh.write("| `%s` | %s | %s | %s |\n" % (k, d.get("VGPRs"), d.get("ScratchSize"), d.get("Occupancy")))
        fh.write("\nThe classical baseline on a scanned sphere (%d scan points, %d cells): share of cells whose label equals the majority label of\n"
                 "`build_cell_labels` (100 samples per cell).\n\n| labelling | agreement |\n|---|---|\n" % (base["scan_points"], base["cells"]))
        fh.write("| every cell outside | %.4f |\n" % base["all_outside"])
        for bw in (0, 1, 4):
            fh.write("| visibility votes + `ops.binary_graph_cut`, binary weight %d | %.4f |\n" % (bw, base["cut_binary_weight_%d" % bw]))
        fh.write("\n```\n%s\n```\n" % "\n".join(json.dumps(r) for r in rows + [dict(baseline=base)]))


if __name__ == "__main__":
    main()
