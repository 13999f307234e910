"""Logits -> labels -> interface facets on the GPU (reference processing/generate_mesh.py:61-107).

``extract_interface(prediction, infinite, nfacets)`` reproduces what ``generate`` does between the network output
and the trimesh call: labels of the finite cells (:75), the infinite cell appended as OUTSIDE (:93-99) and the list
of facets whose two cells carry different labels (:101-105) -- two Python loops over all facets in the reference,
three small kernels here.  The optional integer alpha-expansion graph cut (:15-58, third-party ``gco``) runs exactly on
the device with ``graph_cut.solver: gpu`` (``graph_cut_gpu``), and the iou / chamfer metrics with ``evaluation.solver: gpu``
(``iou_gpu`` / ``chamfer_gpu``), and the mesh object with its watertight and components metrics and the small-component filter with
``mesh.solver: gpu`` (``mesh_gpu`` / ``watertight_gpu`` / ``mesh_components_gpu``), where ``mesh.manifold: repair`` also relabels cells until the
surface is manifold (``manifold_repair_gpu``); without that key the ``trimesh`` mesh object stays a CPU-side third-party step.  ``labels`` can be replaced by the graph-cut labels before ``interface_from_labels``.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .._lib import check, lib, on_device_of, ptr, stream_ptr


@on_device_of
def _compact(values, keep, invert):
    n = keep.numel()
    out = torch.empty(max(n, 1), dtype=torch.int32, device=keep.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=keep.device)
    scratch = torch.empty(int(lib().dgnn_compact_scratch_elems(n)), dtype=torch.int32, device=keep.device)
    check(lib().dgnn_compact_i32(ptr(values), ptr(keep), int(invert), n, ptr(out), ptr(cnt), ptr(scratch), stream_ptr()),
          "dgnn_compact_i32")
    return out[:int(cnt.item())]


@on_device_of
def labels_of_finite_cells(prediction: torch.Tensor, infinite: torch.Tensor) -> torch.Tensor:
    """int32 labels (0 inside / 1 outside) of the cells with infinite == 0, in cell order (reference :75)."""
    if not prediction.is_cuda:
        raise RuntimeError("prediction must be on the GPU")
    prediction = prediction.contiguous()
    n = prediction.size(0)
    labels = torch.empty(n, dtype=torch.int32, device=prediction.device)
    check(lib().dgnn_argmax_rows(ptr(prediction), prediction.size(1), n, prediction.size(1), ptr(labels), stream_ptr()), "dgnn_argmax_rows")
    return _compact(labels, infinite.to(prediction.device, torch.int32).contiguous(), invert=True)


@on_device_of
def interface_from_labels(labels_finite: torch.Tensor, nfacets: torch.Tensor) -> torch.Tensor:
    """Indices (int32, ascending) of the facets whose two cells differ; cell -1 is the outside cell (:93-105)."""
    nfacets = nfacets.to(labels_finite.device, torch.int32).contiguous()
    f = nfacets.size(0)
    flags = torch.empty(max(f, 1), dtype=torch.int32, device=labels_finite.device)[:f]
    check(lib().dgnn_interface_flags(ptr(nfacets), ptr(labels_finite.contiguous()), f, ptr(flags), stream_ptr()), "dgnn_interface_flags")
    return _compact(None, flags, invert=False)


def extract_interface(prediction: torch.Tensor, infinite: torch.Tensor, nfacets: torch.Tensor):
    """-> (labels_finite int32 [Nf], interface facet ids int32 [n_interface])"""
    labels = labels_of_finite_cells(prediction, infinite)
    return labels, interface_from_labels(labels, nfacets)


# ---- reference entry point (processing/generate_mesh.py:61-165) ------------------------------------------------------------
class InterfaceMesh:
    """What `generate` returns as the mesh when trimesh is not installed: the interface triangles as plain arrays, with the
    one method the callers use (`export`, run.py:191 / learning/runModel.py:360).  With trimesh present `generate` returns a
    trimesh.Trimesh built exactly as the reference does (:107-111)."""

    def __init__(self, vertices: np.ndarray, faces: np.ndarray):
        self.vertices = np.asarray(vertices, dtype=np.float64)
        self.faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)

    def export(self, path: str):
        """binary little-endian PLY (vertices double x/y/z, faces as uchar-count int32 lists)"""
        v, f = self.vertices, self.faces.astype(np.int32)
        with open(path, "wb") as fh:
            fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                      "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f))).encode())
            fh.write(np.ascontiguousarray(v, dtype="<f8").tobytes())
            rec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
            rec["n"] = 3
            rec["i"] = f
            fh.write(rec.tobytes())
        return path


def graph_cut(labels, prediction, edges, clf):
    """The reference's alpha-expansion smoothing (:15-58) with its INTEGER costs: unary = round(swapped logits *
    graph_cut.unary_weight), Potts smoothness * binary_weight.  The solver is the third-party `gco` wrapper (un-vendored,
    environment.yml:115) and stays on the CPU; ImportError propagates to `generate`, which falls back to the raw labels
    exactly as the reference's bare `except` does (:88-91)."""
    import gco  # noqa: F401  (gco-wrapper 3.0.8)

    dtype = np.int64
    gc = gco.GCO()
    gc.create_general_graph(int(edges.max()) + 1, 2, energy_is_float=False)
    pred = np.asarray(prediction, dtype=np.float64)[:, [1, 0]]
    gc.set_data_cost(np.array((pred * clf.graph_cut.unary_weight).round(), dtype=dtype))
    gc.set_smooth_cost((1 - np.eye(2)).astype(dtype))
    gc.set_all_neighbors(edges[:, 0], edges[:, 1], np.ones(edges.shape[0], dtype=dtype) * clf.graph_cut.binary_weight)
    for i, l in enumerate(labels):
        gc.init_label_at_site(i, l)
    gc.expansion()
    return gc.get_labels()


def graph_cut_gpu(labels, prediction, edges, clf, row_weights=None):
    """`graph_cut` solved exactly on the device (dgnn_graph_cut_binary): same arguments, same energy.  With two labels and a
    non-negative Potts weight the energy is submodular and gco's converged alpha-expansion is a global minimum, so the minimum cut
    reaches the energy gco reaches; where several labellings share it, the one with the fewest outside cells is returned.
    `prediction` fp32 [Nf, 2] logits of the finite cells (a GPU tensor is read in place), `edges` [F, 2] finite-finite facets,
    clf.graph_cut.unary_weight / binary_weight as in the reference.  `labels` is only checked for its length (the solver needs no
    initial labelling).  Returns what it was given: an ndarray of int32 labels for an ndarray / list `labels` (as gco's
    get_labels), an int32 tensor on the device for a tensor.
    `row_weights` (int [F], one capacity per row of `edges`, e.g. `facet_weights_gpu`): the cut charges row r its own weight instead of
    clf.graph_cut.binary_weight (dgnn_graph_cut_weighted)."""
    from ..ops import binary_graph_cut, weighted_graph_cut

    n = len(labels)
    if n != len(prediction):
        raise ValueError("graph cut: %d labels for %d finite cells" % (n, len(prediction)))
    if not isinstance(prediction, torch.Tensor):
        prediction = torch.from_numpy(np.ascontiguousarray(prediction, dtype=np.float32))
    if not isinstance(edges, torch.Tensor):
        edges = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.int32))
    if row_weights is None:
        lab, _, _ = binary_graph_cut(prediction, edges, clf.graph_cut.unary_weight, clf.graph_cut.binary_weight)
    else:
        lab, _, _ = weighted_graph_cut(prediction, edges, clf.graph_cut.unary_weight, row_weights)
    return lab if isinstance(labels, torch.Tensor) else lab.cpu().numpy()


def _binary_term(clf):
    """clf.graph_cut.binary_term -> None (the reference's uniform weights), "area" or "beta"; the two need ``graph_cut.solver: gpu``"""
    gc = getattr(clf, "graph_cut", None)
    term = getattr(gc, "binary_term", None)
    if term is None or term == "uniform":
        return None
    if term not in ("area", "beta"):
        raise ValueError("graph_cut.binary_term: %r (expected null, \"uniform\", \"area\" or \"beta\")" % (term,))
    if getattr(gc, "solver", None) != "gpu":
        raise ValueError("graph_cut.binary_term: %r needs graph_cut.solver: gpu (no weights are passed to the CPU solver)" % (term,))
    return term


def facet_weights_gpu(mdata, term, binary_weight, device=None):
    """int32 capacities [F] on the device for every facet of the tetrahedralization `mdata` (`_3dt.npz`): ops.facet_cut_terms with
    kind `term` ("area" / "beta") and clf.graph_cut.binary_weight as the scale; 0 for a facet with an infinite cell."""
    from ..ops import facet_cut_terms

    vertices = mdata["vertices"] if device is None else torch.from_numpy(np.ascontiguousarray(mdata["vertices"], dtype=np.float64)).to(device)
    return facet_cut_terms(vertices, mdata["tetrahedra"], mdata["facets"], mdata["nfacets"], term, binary_weight)[0]


def _occupancy_file(data):
    """The reference's lookup (:129-137): data["ioufile"] when it is set, else eval/points.npz, else eval/<id or category>/points.npz"""
    if "ioufile" in data and data["ioufile"]:
        return os.path.join(data.path, data["ioufile"])
    if os.path.exists(os.path.join(data.path, "eval", "points.npz")):
        return os.path.join(data.path, "eval", "points.npz")
    subfolder = data['id'] if data['id'] else data['category']
    return os.path.join(data.path, "eval", subfolder, "points.npz")


def iou_gpu(data, mdata, labels):
    """The reference's `iou` (:127-145) on the device: ONet's points.npz (`points`, bit-packed `occupancies`, unpacked and cut to
    len(points)) against the labelled tetrahedralization `mdata` (`_3dt.npz`) with the finite cells' labels `labels` (0 = inside).  A
    point is inside the reconstructed surface iff the finite cell that contains it is labelled inside; the ratio is
    compute_iou's.  Raises on failure (`generate` turns that into the reference's warning and 0.0)."""
    from ..ops import mesh_iou

    occ = np.load(_occupancy_file(data))
    points = np.asarray(occ["points"], dtype=np.float32)
    gt = np.unpackbits(occ["occupancies"])[:len(points)]
    dev = labels.device if isinstance(labels, torch.Tensor) and labels.is_cuda else None
    if dev is not None:
        points = torch.from_numpy(points).to(dev)
    iou, _, _, _ = mesh_iou(mdata["vertices"], mdata["tetrahedra"], mdata["facets"], mdata["nfacets"], labels, points, gt)
    return iou


def load_occupancy(path):
    """ONet's points.npz -> (points as stored: fp16 / fp32 / fp64 [n, 3], ground-truth occupancies uint8 [n]: the bit-packed
    `occupancies` unpacked and cut to len(points), the reference's :138-139)"""
    occ = np.load(path)
    points = np.asarray(occ["points"])
    if points.dtype not in (np.float16, np.float32, np.float64):
        points = points.astype(np.float32)
    return points, np.unpackbits(occ["occupancies"])[:len(points)]


def iou_mesh_gpu(data, vertices, faces, device=None):
    """The reference's `iou` by its literal method (:139-141): check_mesh_contains of the MESH (vertices [V, 3], faces [F, 3]: any mesh,
    not only an interface of the tetrahedralization) at the points of points.npz, on the device (ops.mesh_occupancy_iou), against the
    file's occupancies.  Selected in `generate` by ``evaluation.occupancy: mesh`` next to ``evaluation.solver: gpu``."""
    from ..ops import mesh_occupancy_iou

    points, gt = load_occupancy(_occupancy_file(data))
    if device is not None:
        points = torch.from_numpy(points).to(device)
    return mesh_occupancy_iou(vertices, faces, points, gt)[0]


def chamfer_gpu(data, mdata, interfaces, clf):
    """The reference's `chamfer` (:147-159, compute_chamfer) on the device: len(gt) points sampled on the interface facets by area
    (seed clf.evaluation.seed, default 0) against eval/<id or category>/pointcloud.npz, exact nearest neighbours both ways.  An interface
    without faces returns inf with a warning (the reference would crash in recon_mesh.sample).  Raises on other failures."""
    from ..ops import chamfer_distance, sample_interface

    subfolder = data['id'] if data['id'] else data['category']
    gt_points = np.load(os.path.join(data.path, "eval", subfolder, "pointcloud.npz"))["points"].astype(np.float32)
    if len(interfaces) == 0:
        print("WARNING: Mesh {} has no faces; Chamfer distance set to inf".format(getattr(data, "filename", "")))
        return float("inf")
    seed = getattr(getattr(clf, "evaluation", None), "seed", None) or 0
    recon_points, _ = sample_interface(mdata["vertices"], mdata["facets"], interfaces, len(gt_points), seed=seed)
    return chamfer_distance(torch.from_numpy(gt_points).to(recon_points.device), recon_points)


SURFACE_METRIC_NAMES = ("accuracy", "completeness", "fscore", "normal_consistency", "hausdorff")


def _fscore_thresholds(clf):
    from .evaluate_mesh import DEFAULT_FSCORE_THRESHOLDS

    value = getattr(getattr(clf, "evaluation", None), "fscore_thresholds", None)
    return [float(t) for t in value] if value is not None else list(DEFAULT_FSCORE_THRESHOLDS)


def surface_metrics_gpu(data, vertices, faces, clf, names):
    """The metrics `names` (within SURFACE_METRIC_NAMES) of the mesh (vertices [V, 3], faces int32 [F, 3] on the device) against
    eval/<id or category>/pointcloud.npz (`points`, `normals`): evaluate_mesh.pointcloud_metrics with seed clf.evaluation.seed and the
    thresholds clf.evaluation.fscore_thresholds (default 0.01, 0.02).  -> dict: the names as keys; for "fscore" the value at the FIRST
    threshold, and "fscore@t", "precision@t", "recall@t" for every threshold t.  Raises on failure."""
    from ..ops import metric_key
    from .evaluate_mesh import pointcloud_metrics

    subfolder = data['id'] if data['id'] else data['category']
    cloud = np.load(os.path.join(data.path, "eval", subfolder, "pointcloud.npz"))
    thresholds = _fscore_thresholds(clf)
    seed = getattr(getattr(clf, "evaluation", None), "seed", None) or 0
    v = torch.as_tensor(np.asarray(vertices, dtype=np.float64)).to(faces.device)
    m = pointcloud_metrics(v, faces, cloud["points"], cloud["normals"] if "normals" in cloud else None, thresholds, seed=seed,
                           name=getattr(data, "filename", ""))
    out = dict()
    for name in names:
        if name == "fscore":
            if thresholds:
                out["fscore"] = m[metric_key("fscore", thresholds[0])]
            out.update({k: x for k, x in m.items() if "@" in k})
        else:
            out[name] = m[name]          # (normal_consistency without `normals` in the file: a KeyError, i.e. the caller's warning)
    return out


def _gpu_surface_metrics(data, clf, vertices, faces, metrics, eval_dict):
    """the surface metrics among `metrics` into eval_dict; a failure warns in the reference's style and writes inf (distances) or 0.0 (scores)"""
    names = [m for m in SURFACE_METRIC_NAMES if m in metrics]
    if not names:
        return
    try:
        eval_dict.update(surface_metrics_gpu(data, vertices, faces, clf, names))
    except Exception:  # noqa: BLE001  (the reference: bare except, :157-159)
        print("WARNING: Could not calculate surface metrics for mesh ", data['filename'])
        from ..ops import metric_key

        for name in names:
            eval_dict[name] = float("inf") if name in ("accuracy", "completeness", "hausdorff") else 0.0
        if "fscore" in names:          # the same keys as on success
            for t in _fscore_thresholds(clf):
                eval_dict.update({metric_key(k, t): 0.0 for k in ("fscore", "precision", "recall")})


def _components_rule(value):
    """clf.mesh.components -> None (no filter), "largest" or an int n >= 1 (components with at least n faces)"""
    if value is None:
        return None
    if value == "largest":
        return "largest"
    if isinstance(value, (int, np.integer)) and not isinstance(value, bool) and int(value) >= 1:
        return int(value)
    raise ValueError("mesh.components: %r (expected null, \"largest\" or an int >= 1)" % (value,))


def mesh_gpu(mdata, labels, interfaces, fix_orientation, components=None, name=""):
    """The mesh `generate` returns, built on the device: the interface facets `interfaces` (int32 ids into mdata["facets"],
    e.g. interface_from_labels) of the labelled tetrahedralization `mdata` (`_3dt.npz`; labels of the finite cells, 0 = inside), wound so
    that every normal points away from its inside cell when `fix_orientation` is set (ops.orient_interface: exact signs; a facet between
    flat cells keeps its stored winding and is counted), else in the stored winding; then only the vertices the faces reference, in
    ascending id, with the faces renumbered (ops.compact_vertices).  Runs on the device of `labels` / `interfaces`.
    `components` ("largest" or an int n >= 1) drops, before the vertex compaction, every face outside the largest connected
    component / in a component of fewer than n faces (ops.mesh_components / mesh_component_measures / filter_components; face order kept).
    Any other value is a ValueError (a configuration mistake); a failing device step warns and leaves the mesh unfiltered.
    -> InterfaceMesh, with more attributes: vertex_ids (the kept original ids, int32 ndarray), n_undetermined, faces_dev (the faces on
    the device), n_removed_faces and keep_mask (bool tensor over `interfaces` on the device; None when nothing was filtered)."""
    from ..ops import compact_vertices, filter_components, mesh_component_measures, mesh_components, orient_interface

    rule = _components_rule(components)
    faces, n_undetermined = orient_interface(mdata["vertices"], mdata["tetrahedra"], mdata["facets"], mdata["nfacets"], labels, interfaces,
                                             orient=bool(fix_orientation))
    n_removed, keep = 0, None
    if rule is not None:
        try:
            comp, k = mesh_components(faces, len(mdata["vertices"]))
            counts = mesh_component_measures(mdata["vertices"], faces, comp, k)["n_faces"]
            kept_faces, keep, n_kept = filter_components(faces, comp, counts, largest=rule == "largest", min_faces=None if rule == "largest" else rule)
            n_removed, faces = faces.shape[0] - n_kept, kept_faces
        except Exception:  # noqa: BLE001  (the reference's style: warn and go on)
            print("WARNING: Could not filter the components of mesh {}. Using the unfiltered mesh.".format(name))
            n_removed, keep = 0, None
    faces, kept = compact_vertices(faces, len(mdata["vertices"]))
    ids = kept.cpu().numpy()
    mesh = InterfaceMesh(np.asarray(mdata["vertices"], dtype=np.float64)[ids], faces.cpu().numpy())
    mesh.vertex_ids, mesh.n_undetermined, mesh.faces_dev = ids, n_undetermined, faces
    mesh.n_removed_faces, mesh.keep_mask = n_removed, keep
    return mesh


def watertight_gpu(mesh, name=""):
    """Open3D's is_watertight (edge-manifold without boundary, vertex-manifold; the reference's metric, generate_mesh.py:115-124) of an
    InterfaceMesh from mesh_gpu, from the device's edge and vertex counts (ops.mesh_topology) -> 0 / 1.  Self-intersection is not tested:
    the interface of a tetrahedralization cannot intersect itself.  A mesh without faces gives 0 with a warning."""
    from ..ops import mesh_topology

    faces = getattr(mesh, "faces_dev", None)
    if faces is None:
        faces = torch.from_numpy(np.ascontiguousarray(mesh.faces, dtype=np.int32).reshape(-1, 3))
    if faces.shape[0] == 0:
        print("WARNING: Mesh {} has no faces; watertight set to 0".format(name))
        return 0
    return mesh_topology(faces, len(mesh.vertices))["watertight"]


MANIFOLD_COST_CAP = 1 << 20


def _manifold_mode(clf):
    """clf.mesh.manifold -> None (the labels stay as they are) or "repair"; the repair needs ``mesh.solver: gpu``"""
    mode = getattr(getattr(clf, "mesh", None), "manifold", None)
    if mode is None:
        return None
    if mode != "repair":
        raise ValueError("mesh.manifold: %r (expected null or \"repair\")" % (mode,))
    if getattr(clf.mesh, "solver", None) != "gpu":
        raise ValueError("mesh.manifold: \"repair\" needs mesh.solver: gpu (the repair runs on the device only)")
    return mode


def _manifold_cost(clf, prediction_finite):
    """clf.mesh.manifold_cost -> None ("count", the default: every cell costs 1, the fewest cells flip) or, for "margin", int32 [Nf] on the
    device: min(round(|logit 0 - logit 1| * mesh.manifold_cost_scale), 2^20) (scale default 1000) -- the cells the network is least sure of
    flip first.  `prediction_finite`: the logits fp32 [Nf, 2] of the finite cells."""
    kind = getattr(clf.mesh, "manifold_cost", None)
    if kind is None or kind == "count":
        return None
    if kind != "margin":
        raise ValueError("mesh.manifold_cost: %r (expected null, \"count\" or \"margin\")" % (kind,))
    scale = getattr(clf.mesh, "manifold_cost_scale", None)
    scale = 1000.0 if scale is None else float(scale)
    if not scale >= 0.0:
        raise ValueError("mesh.manifold_cost_scale: %r (expected a number >= 0)" % (scale,))
    margin = (prediction_finite[:, 0].double() - prediction_finite[:, 1].double()).abs() * scale
    return torch.nan_to_num(margin, nan=0.0).round().clamp(max=MANIFOLD_COST_CAP).to(torch.int32)


def manifold_repair_gpu(mdata, labels, cost=None):
    """The labels of the finite cells of the tetrahedralization `mdata` (`_3dt.npz`) relabelled until the interface is a closed manifold
    surface or no move is left (ops.manifold_repair on the adjacency of ops.tet_neighbors).  labels: int [Nf] (0 = inside),
    cost: int [Nf] >= 0 or None (all ones).  Runs on the device of `labels`.  -> (labels int32 [Nf] on the device, the op's stats:
    singular_after = the vertices still singular, `stuck`)."""
    from ..ops import manifold_repair, tet_neighbors

    dev = labels.device if isinstance(labels, torch.Tensor) and labels.is_cuda else torch.device("cuda", torch.cuda.current_device())
    tets = torch.from_numpy(np.ascontiguousarray(mdata["tetrahedra"], dtype=np.int32)).to(dev)
    nbr = tet_neighbors(torch.from_numpy(np.ascontiguousarray(mdata["facets"], dtype=np.int32)).to(dev),
                        torch.from_numpy(np.ascontiguousarray(mdata["nfacets"], dtype=np.int32)).to(dev), tets)
    return manifold_repair(tets, nbr, torch.as_tensor(labels).to(dev), len(mdata["vertices"]), cost=cost)


def mesh_components_gpu(mesh):
    """The number of connected components of an InterfaceMesh (faces connected through shared edges; ops.mesh_components):
    what the reference reports from trimesh's body_count.  A mesh without faces has 0."""
    from ..ops import mesh_components

    faces = getattr(mesh, "faces_dev", None)
    if faces is None:
        faces = torch.from_numpy(np.ascontiguousarray(mesh.faces, dtype=np.int32).reshape(-1, 3))
    return mesh_components(faces, len(mesh.vertices))[1]


def generate(data, prediction, clf):
    """Same signature and return value as the reference's processing/generate_mesh.py:61 ``generate(data, prediction, clf)``
    -> ``(mesh, eval_dict)``; what runs where:

    * labels of the finite cells (``log_softmax(prediction[infinite == 0]).argmax(1)``, :75) and the interface facets
      (``labels[f0] != labels[f1]`` over all facets with the infinite cell = outside, :93-105 -- two nested Python loops in
      the reference) run on the GPU (dgnn_argmax_rows / dgnn_interface_flags / dgnn_compact_i32); integer results, identical;
    * the optional graph cut (``clf.temp.graph_cut``): with ``clf.graph_cut.solver == "gpu"`` the exact device solver
      (graph_cut_gpu, on the device logits); otherwise the reference's CPU solver when `gco` imports.  Either way a failure keeps
      the raw labels with the reference's warning.  ``clf.graph_cut.binary_type`` is ignored, as in the reference (:34-40); the key
      ``clf.graph_cut.binary_term`` (absent / None / "uniform": every facet weighs ``binary_weight``) set to "area" or "beta" weighs
      each finite-finite facet by its geometry (facet_weights_gpu: rint(binary_weight * q_f)) and needs the gpu solver;
      any other value, or "area" / "beta" without the gpu solver, raises ValueError;
    * the mesh object is a trimesh.Trimesh (``process=True``, optional fix_normals) when trimesh imports, else an
      InterfaceMesh with the same vertices / faces and an ``export``; the evaluation metrics (watertight / iou / chamfer,
      :115-163) need trimesh + utils/libmesh and are computed only when those import -- otherwise eval_dict stays empty;
    * with ``clf.evaluation.solver == "gpu"`` iou and chamfer come from the device (iou_gpu / chamfer_gpu, no trimesh needed), from the
      labels and interface facets above; the mesh object is the same; with ``clf.evaluation.occupancy == "mesh"`` as well, iou is the
      reference's literal check_mesh_contains of the generated mesh (iou_mesh_gpu) instead of the walk in the tetrahedralization;
    * with ``clf.mesh.solver == "gpu"`` the mesh object is built on the device whether or not trimesh imports (mesh_gpu: exact outward
      orientation under ``fix_orientation``, only the referenced vertices) and watertight comes from the device (watertight_gpu).
      On this path only:
      - ``"components"`` in ``clf.temp.metrics``: ``eval_dict["components"]`` = the number of connected components (faces connected
        through shared edges, mesh_components_gpu) of the mesh that is returned;
      - ``clf.mesh.components``: absent / None = no filter; ``"largest"`` = only the component with the most faces is returned; an int
        n >= 1 = only the components with at least n faces.  The returned mesh, ``watertight`` and ``components`` are those of the
        filtered mesh, and ``eval_dict["n_removed_faces"]`` (also ``mesh.n_removed_faces``) says how many faces went.  With
        ``evaluation.solver: gpu`` iou is then check_mesh_contains of the filtered mesh (iou_mesh_gpu: the walk in the labelled
        tetrahedralization would score the unfiltered labels) and chamfer samples the kept facets only.  Any other value of the
        key raises ValueError; a failing device step warns and returns the unfiltered mesh.
      - ``clf.mesh.manifold``: absent / None = the labels stay as they are; ``"repair"`` = the finite cells' labels (from the arg-max or
        from either graph cut) are relabelled before the interface is extracted until no vertex of the surface is singular or no move is
        left (manifold_repair_gpu), and everything after -- orientation, components, metrics, export -- sees the repaired
        labels.  ``clf.mesh.manifold_cost``: ``"count"`` (default; every cell costs 1, the fewest cells flip) or ``"margin"`` (a cell
        costs min(round(|logit 0 - logit 1| * ``mesh.manifold_cost_scale``), 2^20), scale default 1000: the least certain cells flip
        first).  ``eval_dict["manifold_flipped"]`` = the cells that changed side, ``eval_dict["manifold_stuck"]`` = the vertices still
        singular (warned about once when > 0).  ``"repair"`` without ``mesh.solver: gpu``, and any other value, raises ValueError.
    * with ``clf.evaluation.solver == "gpu"`` the names ``accuracy``, ``completeness``, ``hausdorff``, ``normal_consistency`` and ``fscore``
      in ``clf.temp.metrics`` are computed against ``pointcloud.npz`` (surface_metrics_gpu): on the exported, component-filtered
      faces with ``mesh.solver: gpu``, else on the interface facets; ``fscore`` writes the value at the first threshold of
      ``clf.evaluation.fscore_thresholds`` (default 0.01, 0.02) and ``fscore@t``, ``precision@t``, ``recall@t`` for every threshold.  A
      failure warns and writes inf (distances) or 0.0 (scores, the thresholded keys included); without the gpu solver the names are ignored, as unknown names are.
    """
    dev = prediction.device if prediction.is_cuda else torch.device(getattr(clf.temp, "device", "cuda:0"))
    pred_dev = prediction.to(dev, torch.float32)
    infinite = torch.as_tensor(data.infinite)
    # a scene the loader relabelled (processing/reorder.py): `_3dt.npz` knows the cells in FILE order -- logits and the infinite flags go back to it
    from .reorder import restore_cell_order
    # (found on the object, on the loader's tagged tensors, or -- when those were copied -- in the registry of loaded scenes by path + gtfile)
    pred_dev, prediction = restore_cell_order(pred_dev, data), restore_cell_order(prediction, data)
    infinite = restore_cell_order(infinite, data)
    mfile = os.path.join(data.path, data.gtfile + "_3dt.npz")
    mdata = np.load(mfile)
    nfacets = np.ascontiguousarray(mdata["nfacets"]).astype(np.int32)
    labels_dev = labels_of_finite_cells(pred_dev, infinite)
    assert labels_dev.numel() == len(mdata["tetrahedra"])
    if getattr(clf.temp, "graph_cut", None):
        mask = (nfacets >= 0).all(axis=1)
        term = _binary_term(clf)     # a configuration mistake raises here, outside the try
        try:
            if getattr(getattr(clf, "graph_cut", None), "solver", None) == "gpu":
                finite = (infinite == 0).to(dev)
                if term is None:
                    labels_dev = graph_cut_gpu(labels_dev, pred_dev.detach()[finite], torch.from_numpy(nfacets[mask]), clf)
                else:
                    weights = facet_weights_gpu(mdata, term, clf.graph_cut.binary_weight, device=dev)[torch.from_numpy(mask).to(dev)]
                    labels_dev = graph_cut_gpu(labels_dev, pred_dev.detach()[finite], torch.from_numpy(nfacets[mask]), clf, row_weights=weights)
            else:
                finite = (infinite == 0).to(prediction.device)
                lab = graph_cut(labels_dev.cpu().numpy(), prediction[finite].detach().cpu().numpy(), nfacets[mask], clf)
                labels_dev = torch.as_tensor(np.asarray(lab), dtype=torch.int32, device=dev)
        except Exception:  # noqa: BLE001  (the reference: bare except, :88-91)
            print("WARNING: Graph cut for {} didn't work. Using raw predictions for mesh generation.".format(data.filename))
    manifold = None
    if _manifold_mode(clf):          # a configuration mistake raises here
        cost = _manifold_cost(clf, pred_dev.detach()[(infinite == 0).to(dev)])
        labels_dev, manifold = manifold_repair_gpu(mdata, labels_dev, cost=cost)
    interfaces_dev = interface_from_labels(labels_dev, torch.from_numpy(nfacets))
    interfaces = interfaces_dev.cpu().numpy()
    faces = mdata["facets"][interfaces]
    eval_dict = dict()
    try:
        import trimesh
    except ImportError:
        trimesh = None
    if getattr(getattr(clf, "mesh", None), "solver", None) == "gpu":
        mesh, eval_dict = _generate_gpu_mesh(data, clf, mdata, labels_dev, interfaces_dev, trimesh)
        if manifold is not None:
            eval_dict["manifold_flipped"], eval_dict["manifold_stuck"] = manifold["flipped_cells"], manifold["singular_after"]
            if manifold["singular_after"]:
                print("WARNING: {} vertices of mesh {} stay non-manifold after the repair".format(manifold["singular_after"], getattr(data, "filename", "")))
        return mesh, eval_dict
    if getattr(getattr(clf, "evaluation", None), "solver", None) == "gpu":
        return _generate_gpu_metrics(data, clf, mdata, labels_dev, interfaces_dev, faces, trimesh)
    if trimesh is None:
        wanted = [m for m in ("watertight", "iou", "chamfer") if m in (getattr(clf.temp, "metrics", None) or [])]
        if wanted:
            print("WARNING: trimesh is not installed; mesh metrics {} are not computed for {}".format(wanted, getattr(data, "filename", "")))
        return InterfaceMesh(mdata["vertices"], faces), eval_dict
    recon_mesh = trimesh.Trimesh(mdata["vertices"], faces, process=True)
    if getattr(clf.temp, "fix_orientation", None):
        trimesh.repair.fix_normals(recon_mesh)
    metrics = getattr(clf.temp, "metrics", None) or []
    if "watertight" in metrics:
        eval_dict["watertight"] = int(recon_mesh.is_watertight)
    if "chamfer" in metrics:
        eval_dict["chamfer"] = _chamfer_trimesh(data, recon_mesh)
    return recon_mesh, eval_dict


def _chamfer_trimesh(data, recon_mesh):
    from scipy.spatial import cKDTree
    subfolder = data['id'] if data['id'] else data['category']
    gt_points = np.load(os.path.join(data.path, "eval", subfolder, "pointcloud.npz"))["points"].astype(np.float32)
    recon_points = recon_mesh.sample(gt_points.shape[0], return_index=False)
    d1, _ = cKDTree(recon_points).query(gt_points)
    d2, _ = cKDTree(gt_points).query(recon_points)
    return 0.5 * (float(d1.mean()) + float(d2.mean()))


def _generate_gpu_metrics(data, clf, mdata, labels, interfaces, faces, trimesh):
    """`generate`'s tail with ``evaluation.solver: gpu``: the same mesh object, iou / chamfer from iou_gpu / chamfer_gpu, watertight
    from trimesh as before (skipped with a warning when trimesh is missing).  Failures keep the reference's warnings; a failing
    chamfer gives inf (the reference writes its 0.0 into "iou" there)."""
    metrics = getattr(clf.temp, "metrics", None) or []
    if trimesh is not None:
        mesh = trimesh.Trimesh(mdata["vertices"], faces, process=True)
        if getattr(clf.temp, "fix_orientation", None):
            trimesh.repair.fix_normals(mesh)
    else:
        mesh = InterfaceMesh(mdata["vertices"], faces)
    eval_dict = dict()
    if "watertight" in metrics:
        if trimesh is not None:
            eval_dict["watertight"] = int(mesh.is_watertight)
        else:
            print("WARNING: trimesh is not installed; mesh metrics {} are not computed for {}".format(["watertight"], getattr(data, "filename", "")))
    _gpu_iou_chamfer(data, clf, mdata, labels, interfaces, metrics, eval_dict)
    if any(m in metrics for m in SURFACE_METRIC_NAMES):          # on the interface facets, in the tetrahedralization's own vertices
        facets = torch.from_numpy(np.ascontiguousarray(mdata["facets"], dtype=np.int32)).to(interfaces.device)[interfaces.long()]
        _gpu_surface_metrics(data, clf, mdata["vertices"], facets, metrics, eval_dict)
    return mesh, eval_dict


def _gpu_iou_chamfer(data, clf, mdata, labels, interfaces, metrics, eval_dict):
    if "iou" in metrics:
        try:
            if getattr(getattr(clf, "evaluation", None), "occupancy", None) == "mesh":
                faces = torch.from_numpy(np.ascontiguousarray(mdata["facets"], dtype=np.int32)).to(interfaces.device)[interfaces.long()]
                eval_dict["iou"] = iou_mesh_gpu(data, mdata["vertices"], faces, device=interfaces.device)
            else:
                eval_dict["iou"] = iou_gpu(data, mdata, labels)
        except Exception:  # noqa: BLE001  (the reference: bare except, :142-145)
            print("WARNING: Could not calculate IoU for mesh ", data['filename'])
            eval_dict["iou"] = 0.0
    if "chamfer" in metrics:
        try:
            eval_dict["chamfer"] = chamfer_gpu(data, mdata, interfaces, clf)
        except Exception:  # noqa: BLE001  (the reference: bare except, :157-159)
            print("WARNING: Could not calculate Chamfer distance for mesh ", data['filename'])
            eval_dict["chamfer"] = float("inf")


def _gpu_iou_chamfer_filtered(data, clf, mdata, mesh, kept_interfaces, metrics, eval_dict):
    """iou / chamfer of a mesh whose small components were dropped (``mesh.components``): iou from the occupancy of the filtered MESH,
    chamfer from samples on the kept interface facets `kept_interfaces` only (orient_interface keeps the face order, so the keep mask of
    the faces indexes the interface ids).  The reference's warnings on failure."""
    if "iou" in metrics:
        try:
            eval_dict["iou"] = iou_mesh_gpu(data, mesh.vertices, mesh.faces_dev, device=mesh.faces_dev.device)
        except Exception:  # noqa: BLE001  (the reference: bare except, :142-145)
            print("WARNING: Could not calculate IoU for mesh ", data['filename'])
            eval_dict["iou"] = 0.0
    if "chamfer" in metrics:
        try:
            eval_dict["chamfer"] = chamfer_gpu(data, mdata, kept_interfaces, clf)
        except Exception:  # noqa: BLE001  (the reference: bare except, :157-159)
            print("WARNING: Could not calculate Chamfer distance for mesh ", data['filename'])
            eval_dict["chamfer"] = float("inf")


def _generate_gpu_mesh(data, clf, mdata, labels, interfaces, trimesh):
    """`generate`'s tail with ``mesh.solver: gpu``: the mesh from mesh_gpu, watertight from watertight_gpu; iou / chamfer from the device
    with ``evaluation.solver: gpu``, else chamfer by trimesh's sampler when trimesh imports (as without the key).  A facet whose winding
    could not be decided is reported once; a failing metric keeps the reference's warning."""
    metrics = getattr(clf.temp, "metrics", None) or []
    name = getattr(data, "filename", "")
    rule = getattr(getattr(clf, "mesh", None), "components", None)
    mesh = mesh_gpu(mdata, labels, interfaces, getattr(clf.temp, "fix_orientation", None), components=rule, name=name)
    if mesh.n_undetermined:
        print("WARNING: {} faces of mesh {} lie on flat cells only; they keep their stored winding".format(mesh.n_undetermined, name))
    eval_dict = dict()
    if rule is not None:
        eval_dict["n_removed_faces"] = mesh.n_removed_faces
    if "watertight" in metrics:
        try:
            eval_dict["watertight"] = watertight_gpu(mesh, name)
        except Exception:  # noqa: BLE001  (the reference's style: warn and go on)
            print("WARNING: Could not calculate watertightness for mesh ", name)
            eval_dict["watertight"] = 0
    if "components" in metrics:
        try:
            eval_dict["components"] = mesh_components_gpu(mesh)
        except Exception:  # noqa: BLE001
            print("WARNING: Could not count the components of mesh ", name)
            eval_dict["components"] = 0
    if getattr(getattr(clf, "evaluation", None), "solver", None) == "gpu":
        if mesh.keep_mask is None:
            _gpu_iou_chamfer(data, clf, mdata, labels, interfaces, metrics, eval_dict)
        else:
            _gpu_iou_chamfer_filtered(data, clf, mdata, mesh, interfaces[mesh.keep_mask], metrics, eval_dict)
        _gpu_surface_metrics(data, clf, mesh.vertices, mesh.faces_dev, metrics, eval_dict)          # on the exported (filtered) faces
        return mesh, eval_dict
    wanted = [m for m in ("iou", "chamfer") if m in metrics]
    if trimesh is None:
        if wanted:
            print("WARNING: trimesh is not installed; mesh metrics {} are not computed for {}".format(wanted, name))
    elif "chamfer" in metrics:
        eval_dict["chamfer"] = _chamfer_trimesh(data, trimesh.Trimesh(mesh.vertices, mesh.faces, process=False))
    return mesh, eval_dict
