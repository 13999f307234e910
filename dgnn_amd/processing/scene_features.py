"""Scene preparation on the device: from a triangulation (`<scene>_3dt.npz`) and a scan (points + sensor positions) to the model's input
files `<scene>_cgeom.npz`, `<scene>_cbvf.npz`, `<scene>_fbvf.npz`, with facet_rays `<scene>_cbff.npz`, `<scene>_fbff.npz` (§29) and,
with facet_geometry, `<scene>_fgeom.npz` (§32).

The reference gets these files from an external binary; their definitions here are the ones that reproduce its recorded output for
Ignatius scene 99 (counts and edge lengths exactly, the other columns to the last bits).  The facet-ray files (`_cbff`, `_fbff`) hold the
aggregates of ops.ray_walk, every ray followed through all the cells it crosses: the binary's own walk cannot be recovered from its files
(§25), so the rule is this package's definition (§29), not a reproduction.  `_fgeom` (the edge feature `shape`) is missing from the
reference's data and its four column names are unknown: ops.facet_geometry defines them here (§32: facet area, the two circumsphere cosines
of §23, the beta-skeleton term).  The training target
`<scene>_labels.npz` comes from build_cell_labels and a closed ground-truth mesh; the binary's own sample count and generator
are not known, so its labels are a definition of this package's, not a reproduction.

Rows: the cells of a scene are its finite tets in `tetrahedra` order with the infinite cells interleaved where `infinite` is 1; finite
cell number r is tet r.  Infinite cells hold 0 in every column.  Edge row 4 c + k belongs to the facet of cell c opposite its vertex k (the
row order of `_adjacencies.npz`).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops

CGEOM_KEYS = ("radius", "vol", "longest_edge", "shortest_edge")
FGEOM_KEYS = ops.FGEOM_KEYS          # the key order of `_fgeom.npz`
VF_GROUPS = ("inside", "outside", "last")          # the files' key order; `last` holds 0 everywhere
VF_STATS = ("count", "dist_min", "dist_max", "dist_sum")
FF_CELL_GROUPS = tuple("%s_%s" % (g, w) for g in VF_GROUPS for w in ("first", "second"))          # the key order of `_cbff.npz`


def match_vertices(vertices, points):
    """vertex id of every point by exact coordinate match (int64 [P], -1 = no vertex; equal vertices: the lowest id).  Host-side bookkeeping
    on the raw fp64 bits (0.0 and -0.0 are one coordinate)."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    if len(v) == 0:
        return np.full(len(p), -1, dtype=np.int64)
    key = lambda x: (x + 0.0).view(np.dtype((np.void, 24))).reshape(-1)
    kv, kp = key(v), key(p)
    order = np.argsort(kv, kind="stable")
    pos = np.minimum(np.searchsorted(kv[order], kp), len(v) - 1)
    return np.where(kv[order][pos] == kp, order[pos], -1).astype(np.int64)


def build_scene_features(mdata, infinite, scan_points, sensor_position, out_base=None, device=None, facet_rays=False, outside_depth=0, inside_depth=1,
                         facet_geometry=False):
    """mdata: the arrays of `<scene>_3dt.npz` (vertices, tetrahedra, facets, nfacets); infinite [n_cells]: 1 = infinite cell (the
    `infinite` of `_labels.npz`); scan_points, sensor_position [P, 3]: every point that equals a vertex casts that vertex's ray towards its
    sensor, points that share a vertex cast one ray (the lowest-index point's).  Runs ops.tet_neighbors / cell_geometry / vertex_ray_features on
    `device` (default: the current GPU) and returns a dict:
      "cgeom", "cbvf", "fbvf": key -> fp64 ndarray, with the reference files' keys in their order ([n_cells] / [4 n_cells] rows);
      "neighbors": int64 ndarray [n_cells, 4], the cell across each facet of the finite cells (-1: an infinite cell; infinite rows: -1);
      "mean_edge": the loader's mean_edge, "stats": the ray stats plus "points", "unmatched_points", "n_flat".
    With facet_rays also ops.ray_walk(outside_depth, inside_depth) over the same rays, and in the result
      "cbff": cb_facet_{inside,outside,last}_{first,second}_{count,dist_min,dist_max,dist_sum} [n_cells]: per cell the distances at which the
      rays that cross it (after their start cell) enter and leave; "fbff": fb_facet_{inside,outside,last}_... [4 n_cells]: per facet of the
      cell a ray leaves; the `last` groups hold 0, as the vertex family's do; "walk_stats": the stats of ops.ray_walk.
    With facet_geometry also ops.facet_geometry, and in the result
      "fgeom": FGEOM_KEYS -> fp64 ndarray [4 n_cells] (area, cos_own, cos_neighbor, beta per facet of the cell);
      "fgeom_stats": the stats of ops.facet_geometry.  ValueError when they count other than 4 rows per tetrahedron: the `_3dt` does not
      list every facet of every finite cell once.
    With out_base the files are written as out_base + "_cgeom.npz" etc., readable by the reference's and this package's dataLoader."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    inf = np.asarray(infinite).astype(bool).reshape(-1)
    cell_of_tet = np.nonzero(~inf)[0]
    vertices = np.asarray(mdata["vertices"], dtype=np.float64)
    n_cells, n_tets = len(inf), len(mdata["tetrahedra"])
    if len(cell_of_tet) != n_tets:
        raise ValueError("%d finite cells in `infinite` but %d tetrahedra" % (len(cell_of_tet), n_tets))
    vid = match_vertices(vertices, scan_points)
    hit = vid >= 0
    sensors = np.asarray(sensor_position, dtype=np.float64).reshape(-1, 3)
    if len(sensors) != len(vid):
        raise ValueError("%d sensor positions for %d scan points" % (len(sensors), len(vid)))

    v = torch.from_numpy(vertices).to(dev)
    tets = torch.as_tensor(np.asarray(mdata["tetrahedra"])).to(dev, torch.int32)
    fac, nfac = torch.as_tensor(np.asarray(mdata["facets"])).to(dev), torch.as_tensor(np.asarray(mdata["nfacets"])).to(dev)
    nbr = ops.tet_neighbors(fac, nfac, tets)
    geom = ops.cell_geometry(v, tets)
    ray_vertex, ray_sensor = torch.from_numpy(vid[hit]).to(dev), torch.from_numpy(sensors[hit]).to(dev)
    incidence = ops.vertex_incidence(tets, v.size(0))
    rays = ops.vertex_ray_features(v, tets, ray_vertex, ray_sensor, incidence=incidence)

    def cell_col(t):
        col = np.zeros((n_cells,) + tuple(t.shape[1:]))
        col[cell_of_tet] = t.cpu().numpy()
        return col.reshape(-1)

    cgeom = {k: cell_col(geom[k]) for k in CGEOM_KEYS}
    files = {"cb": {}, "fb": {}}
    for prefix, level in (("cb", "tet"), ("fb", "slot")):
        for g in VF_GROUPS:
            for s in VF_STATS:
                key = "%s_vertex_%s_%s" % (prefix, g, s)
                if g == "last":
                    files[prefix][key] = np.zeros(n_cells * (4 if level == "slot" else 1))
                else:
                    files[prefix][key] = cell_col(rays["%s_%s_%s" % (g, level, s.replace("dist_", ""))])
    nbr_tets = nbr.cpu().numpy().astype(np.int64)
    neighbors = np.full((n_cells, 4), -1, dtype=np.int64)
    neighbors[cell_of_tet] = np.where(nbr_tets >= 0, cell_of_tet[np.maximum(nbr_tets, 0)], -1) if n_tets else nbr_tets
    stats = dict(rays["stats"], points=int(len(vid)), unmatched_points=int((~hit).sum()), n_flat=geom["n_flat"])
    if stats["unmatched_points"]:
        print("build_scene_features: %d of %d scan points match no vertex of the triangulation and cast no ray" % (stats["unmatched_points"], len(vid)))
    out = {"cgeom": cgeom, "cbvf": files["cb"], "fbvf": files["fb"], "neighbors": neighbors, "stats": stats,
           "mean_edge": (geom["sum_longest"] + geom["sum_shortest"]) / (2 * n_cells) if n_cells else float("nan")}
    names = ["cgeom", "cbvf", "fbvf"]
    if facet_rays:
        walk = ops.ray_walk(v, tets, nbr, ray_vertex, ray_sensor, outside_depth=outside_depth, inside_depth=inside_depth, incidence=incidence)
        out["cbff"], out["fbff"], out["walk_stats"] = {}, {}, walk["stats"]
        for g in FF_CELL_GROUPS:
            for s in VF_STATS:
                side, which = g.split("_")
                col = np.zeros(n_cells) if side == "last" else cell_col(walk["%s_cell_%s" % (side, "count" if s == "count" else which + s[4:])])
                out["cbff"]["cb_facet_%s_%s" % (g, s)] = col
        for g in VF_GROUPS:
            for s in VF_STATS:
                out["fbff"]["fb_facet_%s_%s" % (g, s)] = np.zeros(4 * n_cells) if g == "last" else cell_col(walk["%s_slot_%s" % (g, s.replace("dist_", ""))])
        names += ["cbff", "fbff"]
    if facet_geometry:
        fg = ops.facet_geometry(v, tets, fac, nfac)
        if fg["stats"]["rows"] != 4 * n_tets:
            raise ValueError("the facets of the triangulation name %d (cell, slot) rows, its %d tetrahedra have %d: `facets` / `nfacets` do not list every "
                             "facet of every finite cell once" % (fg["stats"]["rows"], n_tets, 4 * n_tets))
        out["fgeom"], out["fgeom_stats"] = {k: cell_col(fg[k].reshape(n_tets, 4)) for k in FGEOM_KEYS}, fg["stats"]
        names.append("fgeom")
    if out_base is not None:
        for name in names:
            np.savez(out_base + "_%s.npz" % name, **out[name])
    return out


def build_cell_labels(mdata, infinite, gt_vertices, gt_faces, n_samples=100, seed=0, out_base=None, device=None):
    """The training target of a scene: the share of every cell inside the closed ground-truth mesh (gt_vertices [M, 3], gt_faces [F, 3]),
    from n_samples points per tet (ops.cell_labels on `device`, default: the current GPU).  mdata and infinite as in build_scene_features.
    Returns a dict: "inside_perc", "outside_perc" fp64 [n_cells] (finite cells: their tets' fractions in tet order; infinite cells: 0 and
    1), "infinite" int32 [n_cells] as given, and "stats": n_samples, n_disagree, the cells with fraction 0 ("n_outside"), 1 ("n_inside")
    and in between ("n_partial", infinite cells not counted) and "watertight" (ops.mesh_topology).  A mesh that is not watertight is
    labelled all the same, after a warning.  With out_base the file out_base + "_labels.npz" is written with the keys inside_perc,
    outside_perc, infinite in this order, as the reference's and this package's dataLoader read it."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    inf = np.asarray(infinite).reshape(-1)
    finite = inf.astype(bool) == 0
    n_cells, n_tets = len(inf), len(mdata["tetrahedra"])
    if int(finite.sum()) != n_tets:
        raise ValueError("%d finite cells in `infinite` but %d tetrahedra" % (int(finite.sum()), n_tets))
    v = torch.from_numpy(np.asarray(mdata["vertices"], dtype=np.float64)).to(dev)
    tets = torch.as_tensor(np.asarray(mdata["tetrahedra"])).to(dev, torch.int32)
    gv = torch.from_numpy(np.asarray(gt_vertices, dtype=np.float64)).to(dev)
    gf = torch.as_tensor(np.asarray(gt_faces)).to(dev, torch.int32)
    lab = ops.cell_labels(gv, gf, v, tets, n_samples=n_samples, seed=seed)
    try:
        watertight = ops.mesh_topology(gf, gv.size(0))["watertight"]
    except ops.DgnnError:          # a face with a repeated vertex
        watertight = 0
    if not watertight:
        print("Warning: the ground-truth mesh is not watertight; its cell labels follow the ray parities all the same.")
    if lab["n_disagree"]:
        print("Warning: contains1 != contains2 for %d of %d samples (counted as outside)." % (lab["n_disagree"], n_tets * lab["n_samples"]))
    inside, outside = np.zeros(n_cells), np.ones(n_cells)
    inside[finite], outside[finite] = lab["inside_perc"].cpu().numpy(), lab["outside_perc"].cpu().numpy()
    count = lab["count"].cpu().numpy()
    stats = dict(n_samples=lab["n_samples"], n_disagree=lab["n_disagree"], n_outside=int((count == 0).sum()), n_inside=int((count == lab["n_samples"]).sum()),
                 watertight=int(watertight))
    stats["n_partial"] = n_tets - stats["n_outside"] - stats["n_inside"]
    out = {"inside_perc": inside, "outside_perc": outside, "infinite": inf.astype(np.int32), "stats": stats}
    if out_base is not None:
        np.savez(out_base + "_labels.npz", inside_perc=out["inside_perc"], outside_perc=out["outside_perc"], infinite=out["infinite"])
    return out
