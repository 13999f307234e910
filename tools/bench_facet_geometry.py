"""Times the `_fgeom` columns on the device -- ops.facet_geometry, split into its sphere pass (ops.cell_circumspheres) and its facet pass
(ops.facet_geometry on the stored spheres) -- next to ops.facet_cut_terms(kind="beta"), the recompute-form sibling over the finite-finite
facets, and next to the numpy model of tests/facet_geometry_model.py on the same host (timed once: a model, not tuned
code).  Scenes: the Ignatius fixture (tests/golden/ignatius_3dt.npz with the facets of the scene-features fixture) and the exact Delaunay
triangulation of --points seeded uniform points by ops.delaunay (150 000 points: about 1M tets).  In every repetition the four device calls
run in turn, so they share whatever else the host is doing; every timing is the host clock around one whole Python call ending in a device
synchronise.  The device results are checked against the model's bit for bit.  Prints one JSON line per scene; --out also gets the table.

    python tools/bench_facet_geometry.py [--points 150000] [--reps 20] [--out FILE] [--scenes ignatius,delaunay] [--no-model]
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

import facet_geometry_model as fgm  # noqa: E402
import scene_features_model as sf  # noqa: E402
from dgnn_amd import ops  # noqa: E402

CALLS = ("facet_geometry", "sphere_pass", "facet_pass", "cut_terms_beta")


def compulsory_bytes(scene):
    """-> dict of the bytes each pass cannot avoid.  Sphere pass: every cell's row of `tetrahedra` (16 B) and its record (32 B, written), every
    vertex once (24 B).  Facet pass: every facet's `nfacets` and `facets` rows (8 + 12 B); per side with a cell its row of `tetrahedra` (16 B), its
    record (32 B) and the four values of its output row (32 B, written); every vertex once.  The whole call also zero-fills the 16 T output
    doubles.  cut_terms(beta): the two rows of every facet and its q and w (8 + 4 B, written), per finite-finite side the cell's row; every vertex
    once."""
    t, f, v = len(scene["tetrahedra"]), len(scene["facets"]), len(scene["vertices"])
    sides = int((scene["nfacets"] >= 0).sum())
    both = int((scene["nfacets"] >= 0).all(axis=1).sum())
    sphere = 48 * t + 24 * v
    facet = 20 * f + 80 * sides + 24 * v
    return dict(sphere_pass=sphere, facet_pass=facet, facet_geometry=sphere + facet + 128 * t, cut_terms_beta=32 * f + 32 * both + 24 * v)


def _summary(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def bench(name, scene, reps, model):
    d = {k: torch.from_numpy(np.ascontiguousarray(scene[k])).cuda() for k in ("vertices", "tetrahedra", "facets", "nfacets")}
    args = (d["vertices"], d["tetrahedra"], d["facets"], d["nfacets"])
    sph = ops.cell_circumspheres(d["vertices"], d["tetrahedra"])
    calls = {"facet_geometry": lambda: ops.facet_geometry(*args), "sphere_pass": lambda: ops.cell_circumspheres(d["vertices"], d["tetrahedra"]),
             "facet_pass": lambda: ops.facet_geometry(*args, spheres=sph), "cut_terms_beta": lambda: ops.facet_cut_terms(*args, "beta", 10.0, return_q=True)}
    for _ in range(3):          # warm-up: code objects, the allocator's blocks of every size used below
        for k in CALLS:
            calls[k]()
    ms, out = {k: [] for k in CALLS}, {}
    for _ in range(reps):
        for k in CALLS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[k] = calls[k]()
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0))
    nbytes = compulsory_bytes(scene)
    res = dict(scene=name, vertices=len(scene["vertices"]), tets=len(scene["tetrahedra"]), facets=len(scene["facets"]), reps=reps,
               stats=out["facet_geometry"]["stats"], cut_terms_stats=out["cut_terms_beta"][2], bytes=nbytes,
               ms={k: _summary(ms[k]) for k in CALLS},
               gb_per_s_of_the_whole_call={k: nbytes[k] / (1e6 * float(np.median(ms[k]))) for k in CALLS})
    bits = lambda x: np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64).view(np.int64)
    both = (scene["nfacets"] >= 0).all(axis=1)
    rows = fgm.facet_rows(scene)
    beta, q = out["facet_geometry"]["beta"].cpu().numpy(), out["cut_terms_beta"][1].cpu().numpy()
    res["beta_equals_cut_terms_q"] = bool(all(np.array_equal(bits(beta[rows[both, s]]), bits(q[both])) for s in (0, 1)))
    res["two_calls_equal_one"] = bool(all(torch.equal(out["facet_geometry"][k], out["facet_pass"][k]) for k in fgm.FGEOM_KEYS))
    if model:
        t0 = time.perf_counter()
        m_sph = fgm.cell_circumspheres(scene["vertices"], scene["tetrahedra"])
        t1 = time.perf_counter()
        m = fgm.facet_geometry(scene)
        t2 = time.perf_counter()
        res["model_ms"] = dict(sphere_pass=1e3 * (t1 - t0), facet_geometry=1e3 * (t2 - t1))
        res["matches_model"] = bool(all(np.array_equal(bits(out["facet_geometry"][k]), bits(m[k])) for k in fgm.FGEOM_KEYS)
                                    and np.array_equal(bits(out["sphere_pass"]["records"][:, 3]), bits(m_sph["radius"]))
                                    and out["facet_geometry"]["stats"] == m["stats"])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="a file for the table and the JSON lines (profiles/facet_geometry.md holds those of the recorded run)")
    ap.add_argument("--no-model", action="store_true", help="skip the numpy model (and the check against it): for a run under a profiler")
    ap.add_argument("--scenes", default="ignatius,delaunay", help="which of the two scenes to run (a kernel trace of one scene has one size per kernel)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_facet_geometry needs a GPU")
    from dgnn_amd.processing.triangulate import triangulate_scan
    rows = []
    if "ignatius" in a.scenes.split(","):
        fx, g = sf.load_fixture(), np.load(os.path.join(ROOT, "tests", "golden", "ignatius_3dt.npz"))
        rows.append(bench("ignatius", dict(vertices=np.asarray(g["vertices"], np.float64), tetrahedra=np.asarray(g["tetrahedra"], np.int32),
                                           facets=np.asarray(fx["facets"], np.int32), nfacets=np.asarray(fx["nfacets"], np.int32)), a.reps, not a.no_model))
    if "delaunay" in a.scenes.split(","):
        rows.append(bench("delaunay_%d" % a.points, triangulate_scan(np.random.default_rng(0).random((a.points, 3)))["mdata"], a.reps, not a.no_model))
    if a.out is None:
        return
    with open(a.out, "w") as fh:
        fh.write("| scene | tets | facets | call | device, median of %d (min .. max), ms | compulsory MB | MB / median ms = GB/s of the whole call | numpy model, once, ms |\n"
                 "|---|---|---|---|---|---|---|---|\n" % a.reps)
        for r in rows:
            for k in CALLS:
                model = r.get("model_ms", {}).get(k)
                fh.write("| %s | %d | %d | `%s` | %.3f (%.3f .. %.3f) | %.2f | %.1f | %s |\n" % (
                    r["scene"], r["tets"], r["facets"], k, r["ms"][k]["median"], r["ms"][k]["min"], r["ms"][k]["max"], r["bytes"][k] / 1e6,
                    r["gb_per_s_of_the_whole_call"][k], "%.0f" % model if model is not None else "--"))
        fh.write("\n```\n%s\n```\n" % "\n".join(json.dumps(r) for r in rows))


if __name__ == "__main__":
    main()
