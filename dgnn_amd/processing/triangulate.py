"""From a scan to a scene folder: the triangulator between scan_mesh and build_scene_features / build_cell_labels; make_scene
chains all of them, with facet_rays through the facet-ray walk and with facet_geometry through ops.facet_geometry (§32) as well.

The reference gets `<scene>_3dt.npz` and `<scene>_adjacencies.npz` from an external binary; here they come from ops.delaunay -- the exact
Delaunay triangulation of the scan's distinct points with one infinite cell per hull facet.

Cells: the T finite cells in `tetrahedra` order, then the H infinite cells in the order of ops.delaunay (by finite cell and slot); `infinite` is
T zeros and H ones.  `_adjacencies.npz` row 4 c + k is (c, the cell across the facet opposite vertex k of c); for an infinite cell slot 0 is
its finite cell and slots 1..3 the infinite cells across the three edges of its hull facet.  `_3dt.npz` holds every facet of the finite cells
once, in the order of (its lower cell, that cell's slot), with its two cells in finite numbering and -1 for the infinite side.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import ops

_FACET_OF_SLOT = ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))


def drop_duplicates(points):
    """(the distinct points in the order of their first occurrence, the index of each kept point, how many were dropped): equality on the raw
    fp64 bits with 0.0 and -0.0 as one value, the key of scene_features.match_vertices"""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    if len(p) == 0:
        return p, np.zeros(0, dtype=np.int64), 0
    key = (p + 0.0).view(np.dtype((np.void, 24))).reshape(-1)
    _, first = np.unique(key, return_index=True)
    first.sort()
    return p[first], first, len(p) - len(first)


def triangulate_scan(points, out_base=None, priority=None, seed=0, device=None):
    """points [P, 3] (a scan's points; duplicates are dropped, first occurrence kept) -> dict:
      "mdata": vertices fp64 [V, 3], tetrahedra int32 [T, 4], facets int32 [F, 3], nfacets int32 [F, 2] -- the arrays of `_3dt.npz`;
      "adjacencies" int32 [4 N, 2], N = T + H; "infinite" int32 [N]; "neighbors" int32 [N, 4]; "hull_facets" int32 [H, 3];
      "kept" int64 [V]: the input row of every vertex; "n_dropped"; "stats": those of ops.delaunay.
    priority (over the KEPT points) and seed as in ops.delaunay.  With out_base, out_base + "_3dt.npz" and "_adjacencies.npz" are written."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    verts, kept, dropped = drop_duplicates(points)
    tri = ops.delaunay(torch.from_numpy(verts).to(dev), priority=priority, seed=seed)
    tets, nbr = tri["tetrahedra"], tri["neighbors"]
    T, N = tets.size(0), nbr.size(0)
    # a facet is listed by its lower cell; an infinite neighbour (id >= T) is always the higher one
    fin = nbr[:T].long()
    cell = torch.arange(T, device=dev).reshape(T, 1).expand(T, 4)
    own = (fin > cell).reshape(-1)
    slot = torch.tensor(_FACET_OF_SLOT, dtype=torch.int64, device=dev)
    facets = tets.long()[:, slot].reshape(-1, 3)[own]
    other = torch.where(fin >= T, torch.full_like(fin, -1), fin).reshape(-1)[own]
    nfacets = torch.stack([cell.reshape(-1)[own], other], dim=1)
    adj = torch.stack([torch.arange(N, device=dev).repeat_interleave(4), nbr.long().reshape(-1)], dim=1)
    infinite = np.concatenate([np.zeros(T, dtype=np.int32), np.ones(N - T, dtype=np.int32)])
    mdata = dict(vertices=verts, tetrahedra=tets.cpu().numpy(), facets=facets.to(torch.int32).cpu().numpy(),
                 nfacets=nfacets.to(torch.int32).cpu().numpy())
    out = dict(mdata=mdata, adjacencies=adj.to(torch.int32).cpu().numpy(), infinite=infinite, neighbors=nbr.cpu().numpy(),
               hull_facets=tri["hull_facets"].cpu().numpy(), kept=kept, n_dropped=dropped, stats=tri["stats"])
    if out_base is not None:
        np.savez(out_base + "_3dt.npz", **mdata)
        np.savez(out_base + "_adjacencies.npz", adjacencies=out["adjacencies"])
    return out


def make_scene(gt_vertices, gt_faces, out_base, n_samples=100, label_seed=0, priority=None, device=None, facet_rays=False, facet_geometry=False, **scan_args):
    """A closed ground-truth mesh -> every file dataLoader.run opens for node_features within {shape, vertex, count, min, max, sum} and
    edge_features within {vertex, count, min, max, sum}: scan_mesh(**scan_args) -> triangulate_scan -> build_scene_features ->
    build_cell_labels, written as out_base + "_3dt.npz", "_adjacencies.npz", "_cgeom.npz", "_cbvf.npz", "_fbvf.npz", "_labels.npz".
    With facet_rays also "_cbff.npz" and "_fbff.npz" (every ray walked through all its cells): the scene then supports the wider
    sets, node_features within {shape, vertex, facet, ...} and edge_features within {vertex, facet, ...}.  With facet_geometry also
    "_fgeom.npz" (DESIGN §32), the edge feature `shape`; with both flags the folder holds all nine files and loads under the reference's
    shipped lists, edge_features [shape, vertex, facet, count, min, max, sum].  Returns the four stages' results: dict of "scan", "triangulation", "features", "labels"."""
    from .scan_mesh import scan_mesh
    from .scene_features import build_cell_labels, build_scene_features

    folder = os.path.dirname(out_base)
    if folder:
        os.makedirs(folder, exist_ok=True)
    scan = scan_mesh(gt_vertices, gt_faces, device=device, **scan_args)
    tri = triangulate_scan(scan["points"], out_base=out_base, priority=priority, seed=scan_args.get("seed", 0), device=device)
    feat = build_scene_features(tri["mdata"], tri["infinite"], scan["points"], scan["sensor_position"], out_base=out_base, device=device,
                                facet_rays=facet_rays, facet_geometry=facet_geometry)
    lab = build_cell_labels(tri["mdata"], tri["infinite"], gt_vertices, gt_faces, n_samples=n_samples, seed=label_seed, out_base=out_base, device=device)
    return dict(scan=scan, triangulation=tri, features=feat, labels=lab)
