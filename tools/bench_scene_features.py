"""Times the device scene front end -- ops.tet_neighbors, ops.cell_geometry, ops.vertex_incidence, ops.vertex_ray_features -- on a seeded
scipy Delaunay scene at bench scale (150 000 points, about 1M tets; one ray per vertex towards a sensor on a sphere around the scene) and
on the Ignatius fixture (tests/golden/ignatius_scene_features*.npz), next to the numpy model of the same ops on the same host
(tests/scene_features_model.py, timed once: it is a model, not tuned code).  The device results are checked against the model's.
Prints one JSON line per scene and writes the table to --out; every device timing ends in a device synchronise.

    python tools/bench_scene_features.py [--points 150000] [--reps 5] [--out profiles/scene_features.md]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mesh_metrics_model as mm  # noqa: E402
import scene_features_model as sf  # noqa: E402
from dgnn_amd import ops  # noqa: E402

OPS = ("tet_neighbors", "cell_geometry", "vertex_incidence", "vertex_ray_features")


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


def _host_time(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def _bits_equal(t, a):
    return bool(np.array_equal(t.cpu().numpy().astype(np.float64).view(np.int64), np.asarray(a, np.float64).view(np.int64)))


def bench(name, scene, rv, sensors, reps):
    v, tets = torch.from_numpy(scene["vertices"]).cuda(), torch.from_numpy(scene["tetrahedra"]).cuda()
    fac, nfac = torch.from_numpy(scene["facets"]).cuda(), torch.from_numpy(scene["nfacets"]).cuda()
    rv_d, s_d = torch.from_numpy(rv).cuda(), torch.from_numpy(sensors).cuda()
    nv = len(scene["vertices"])
    gpu, host = {}, {}
    nbr, gpu["tet_neighbors"] = _time(lambda: ops.tet_neighbors(fac, nfac, tets), reps)
    geom, gpu["cell_geometry"] = _time(lambda: ops.cell_geometry(v, tets), reps)
    inc, gpu["vertex_incidence"] = _time(lambda: ops.vertex_incidence(tets, nv), reps)
    rays, gpu["vertex_ray_features"] = _time(lambda: ops.vertex_ray_features(v, tets, rv_d, s_d, incidence=inc), reps)
    (m_nbr, _), host["tet_neighbors"] = _host_time(lambda: sf.tet_neighbors(scene["facets"], scene["nfacets"], scene["tetrahedra"]))
    m_geom, host["cell_geometry"] = _host_time(lambda: sf.cell_geometry(scene["vertices"], scene["tetrahedra"]))
    (m_ptr, _), host["vertex_incidence"] = _host_time(lambda: sf.vertex_incidence(scene["tetrahedra"], nv))
    m_rays, host["vertex_ray_features"] = _host_time(lambda: sf.vertex_rays(scene["vertices"], scene["tetrahedra"], rv, sensors))
    same = (np.array_equal(nbr.cpu().numpy(), m_nbr) and np.array_equal(inc[0].cpu().numpy(), m_ptr)
            and all(_bits_equal(geom[k], m_geom[k]) for k in ("radius", "vol", "longest_edge", "shortest_edge"))
            and np.array_equal(rays["ray_tet"].cpu().numpy(), m_rays["ray_tet"]) and _bits_equal(rays["ray_dist"], m_rays["ray_dist"])
            and all(_bits_equal(rays["%s_%s_sum" % (s, lv)], m_rays["%s_%s_sum" % (s, lv)]) for s in sf.SIDES for lv in ("tet", "slot")))
    out = dict(scene=name, vertices=nv, tets=len(scene["tetrahedra"]), facets=len(scene["facets"]), rays=len(rv), matches_model=bool(same),
               ray_stats=rays["stats"])
    out.update({"gpu_%s_ms_median" % k: gpu[k] for k in OPS})
    out.update({"model_%s_ms" % k: host[k] for k in OPS})
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_features.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_features needs a GPU")
    rows = []
    scene = mm.scene_from_points(np.random.default_rng(0).random((a.points, 3)))
    d = np.random.default_rng(1).standard_normal((a.points, 3))
    rows.append(bench("delaunay", scene, np.arange(a.points), 0.5 + 3.0 * d / np.linalg.norm(d, axis=1, keepdims=True), a.reps))
    fx, g = sf.load_fixture(), np.load(os.path.join(ROOT, "tests", "golden", "ignatius_3dt.npz"))
    scene = dict(vertices=g["vertices"], tetrahedra=g["tetrahedra"], facets=fx["facets"], nfacets=fx["nfacets"])
    rows.append(bench("ignatius", scene, sf.match_vertices(g["vertices"], fx["points"]), fx["sensor_position"], a.reps))
    with open(a.out, "w") as fh:
        fh.write("| scene | tets | rays | op | device, median of %d (ms) | numpy model, once (ms) |\n|---|---|---|---|---|---|\n" % a.reps)
        for r in rows:
            for k in OPS:
                fh.write("| %s | %d | %d | `%s` | %.3f | %.1f |\n" % (r["scene"], r["tets"], r["rays"], k, r["gpu_%s_ms_median" % k], r["model_%s_ms" % k]))
        fh.write("\n```\n%s\n```\n" % "\n".join(json.dumps(r) for r in rows))


if __name__ == "__main__":
    main()
