"""The device mesh components (ops.mesh_components / mesh_component_measures / filter_components, the `components` metric and the
``mesh.components`` filter of `generate`, evaluate's topology report) against the CPU model tests/mesh_components_model.py: labels, counts,
keep masks and filtered faces exactly, the fp64 sums within the model's derived bound of math.fsum."""
import functools

import numpy as np
import pytest
import torch

import mesh_components_model as mc
import mesh_metrics_model as mm
import mesh_topology_model as mt
from dgnn_amd.config import Config
from helpers import gold

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = mc.HAND_MADE + ["strip_shuffled", "tets_1000", "shells", "crumbs_then_strip", "gold"]


@functools.lru_cache(maxsize=None)
def _case(which):
    """-> (vertices, faces, the model's comp, K, measures); computed once, read only"""
    if which in mc.HAND_MADE:
        v, f, _ = mc.hand_made(which)
    elif which == "strip_shuffled":
        v, f = mc.strip(4099, seed=1)
    elif which == "tets_1000":
        v, f = mc.many_tets(1000)
    elif which == "shells":
        v, f = mc.shells_and_crumbs()
    elif which == "crumbs_then_strip":
        v, f = mc.crumbs_then_strip()
    else:
        g = gold("genmesh_f4_small.npz")
        v, f = g["vertices"].astype(np.float64), g["faces"].astype(np.int32)
    comp, k = mc.components(f)
    for a in (v, f, comp):
        a.setflags(write=False)
    return v, f, comp, k, mc.measures(v, f, comp, k)


def _t(x):
    return torch.from_numpy(np.array(x)).to(DEV)          # (a copy: the shared cases are read-only)


def _device(v, f):
    from dgnn_amd import ops
    comp, k = ops.mesh_components(_t(f), len(v))
    return comp, k, ops.mesh_component_measures(_t(v), _t(f), comp, k)


@pytest.mark.parametrize("which", CASES)
def test_labels_counts_and_filters_equal_the_model(which):
    from dgnn_amd import ops
    v, f, want, want_k, m = _case(which)
    if which in mc.HAND_MADE:
        assert want_k == mc.hand_made(which)[2]
    comp, k, got = _device(v, f)
    assert comp.dtype == torch.int32 and comp.device.type == "cuda" and comp.shape == (len(f),)
    assert k == want_k and np.array_equal(comp.cpu().numpy(), want)
    assert got["n_faces"].dtype == torch.int64 and np.array_equal(got["n_faces"].cpu().numpy(), m["n_faces"])
    rules = [dict(largest=True), dict(min_faces=1), dict(min_faces=2), dict(min_faces=4), dict(min_faces=5)]
    for rule in rules:
        kept, keep, n = ops.filter_components(_t(f), comp, got["n_faces"], **rule)
        want_kept, want_keep, want_n = mc.filter_faces(f, want, m["n_faces"], **rule)
        assert n == want_n and keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), want_keep), rule
        assert kept.dtype == torch.int32 and np.array_equal(kept.cpu().numpy().reshape(-1, 3), want_kept), rule


@pytest.mark.parametrize("which", CASES)
def test_measures_are_within_the_derived_bound_of_fsum(which):
    v, f, _, _, m = _case(which)
    _, k, got = _device(v, f)
    area, vol = got["area"].cpu().numpy(), got["signed_volume"].cpu().numpy()
    assert area.dtype == np.float64 and area.shape == (k,) and vol.shape == (k,)
    da, dv = np.abs(area - m["area"]), np.abs(vol - m["signed_volume"])
    if k:
        print("%s: K=%d  max |area - fsum| / bound = %.3g   max |volume - fsum| / bound = %.3g" % (
            which, k, (da / m["area_bound"]).max(), (dv / np.maximum(m["volume_bound"], 5e-324)).max()))
    assert (da <= m["area_bound"]).all() and (dv <= m["volume_bound"]).all()
    if which == "crumbs_then_strip":        # the strip's sorted positions [3, 703) start inside a chunk of 256 and cross two boundaries
        assert m["n_faces"].tolist() == [1, 1, 1, 700] and m["area"][3] > 100 * m["area"][:3].max()


@pytest.mark.parametrize("flip", [False, True])
def test_unit_tetrahedron_has_a_sixth_of_volume(flip):
    v, f = mc.unit_tet(flip)
    _, k, got = _device(v, f)
    m = mc.measures(v, f, np.zeros(4, dtype=np.int32), 1)
    want = -1.0 / 6.0 if flip else 1.0 / 6.0
    assert k == 1 and m["signed_volume"][0] == want
    assert abs(got["signed_volume"].item() - want) <= m["volume_bound"][0]
    assert abs(got["area"].item() - (1.5 + np.sqrt(3.0) / 2.0)) <= m["area_bound"][0] + 4 * mc.U * 3   # (+ the rounding of the closed form)


@pytest.mark.parametrize("which", ["strip_shuffled", "tets_1000", "gold"])
def test_two_runs_are_bit_identical(which):
    from dgnn_amd import ops
    v, f, _, _, _ = _case(which)
    runs = []
    for _ in range(2):
        comp, k, got = _device(v, f)
        kept, keep, n = ops.filter_components(_t(f), comp, got["n_faces"], largest=True)
        runs.append([comp.cpu().numpy(), np.int64(k), got["n_faces"].cpu().numpy(), got["area"].cpu().numpy().view(np.int64),
                     got["signed_volume"].cpu().numpy().view(np.int64), kept.cpu().numpy(), keep.cpu().numpy(), np.int64(n)])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


def test_largest_breaks_a_tie_towards_the_smaller_id_and_min_faces_keeps_the_shells():
    from dgnn_amd import ops
    v, f, _, _, m = _case("shells")
    comp, k, got = _device(v, f)
    assert k == 5 and got["n_faces"].tolist() == [4, 1, 4, 1, 1]
    kept, keep, n = ops.filter_components(_t(f), comp, got["n_faces"], largest=True)
    assert n == 4 and np.array_equal(np.nonzero(keep.cpu().numpy())[0], [0, 2, 4, 8])
    kept, keep, n = ops.filter_components(_t(f), comp, got["n_faces"], min_faces=4)
    assert n == 8 and np.array_equal(kept.cpu().numpy(), f[[0, 2, 3, 4, 6, 7, 8, 10]])          # the face order is kept
    fc, ids = ops.compact_vertices(kept, len(v))
    assert ids.tolist() == [0, 1, 2, 3, 10, 11, 12, 13] and np.array_equal(ids.cpu().numpy()[fc.cpu().numpy()], kept.cpu().numpy())
    with pytest.raises(ValueError):
        ops.filter_components(_t(f), comp, got["n_faces"])
    with pytest.raises(ValueError):
        ops.filter_components(_t(f), comp, got["n_faces"], largest=True, min_faces=2)
    with pytest.raises(ValueError):
        ops.filter_components(_t(f), comp, got["n_faces"], min_faces=0)


def test_takes_ndarrays_like_mesh_topology():
    from dgnn_amd import ops
    v, f, want, want_k, m = _case("two_tets")
    v, f = v.copy(), f.copy()                                  # (the shared case is read-only; torch wants writable arrays)
    comp, k = ops.mesh_components(f, len(v))
    got = ops.mesh_component_measures(v, f, comp.cpu().numpy(), k)
    kept, keep, n = ops.filter_components(f, comp.cpu().numpy(), got["n_faces"].cpu().numpy(), largest=True)
    assert k == want_k and np.array_equal(comp.cpu().numpy(), want) and kept.is_cuda and n == 4 and keep.cpu().numpy()[:4].all()


def test_invalid_input_raises_what_mesh_topology_raises():
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    faces = np.array(mt.tetra_faces((0, 1, 2, 3)), dtype=np.int32)
    for call in (ops.mesh_topology, ops.mesh_components):
        with pytest.raises(DgnnError, match="out of range"):
            call(_t(faces), 3)
        with pytest.raises(DgnnError, match="repeated vertex"):
            call(_t(np.array([[0, 1, 1]], dtype=np.int32)), 4)
    v = mc.UNIT_TET
    with pytest.raises(DgnnError, match="out of range"):
        ops.mesh_component_measures(_t(v), _t(faces), _t(np.array([0, 0, 1, 0], dtype=np.int32)), 1)
    with pytest.raises(DgnnError, match="out of range"):
        ops.mesh_component_measures(_t(v[:3]), _t(faces), _t(np.zeros(4, dtype=np.int32)), 1)
    with pytest.raises(DgnnError, match="out of range"):
        ops.mesh_component_measures(_t(v), _t(faces), _t(np.zeros(4, dtype=np.int32)), 0)        # faces, but no components
    with pytest.raises(DgnnError, match="out of range"):
        ops.filter_components(_t(faces), _t(np.array([0, 0, 2, 0], dtype=np.int32)), _t(np.array([3, 1], dtype=np.int64)), min_faces=1)


# ---- generate / evaluate ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _blob_scene():
    """a Delaunay scene labelled by a sphere and a small floating blob of inside cells near a corner -> (scene, labels, sd, the oriented
    interface faces, the model's comp, K, counts)"""
    scene = mm.scene_from_points(np.random.default_rng(3).random((3000, 3)))
    cen = mm.centroids(scene)
    sd = np.minimum(np.linalg.norm(cen - 0.5, axis=1) - 0.3, np.linalg.norm(cen - 0.86, axis=1) - 0.09)
    labels = (sd > 0).astype(np.int32)
    ids = mm.interface_ids(labels, scene["nfacets"])
    faces, _ = mt.orient_interface(scene, labels, ids)
    comp, k = mc.components(faces)
    assert k >= 2, "the scene needs a floating blob"
    return scene, labels, sd, ids, faces, comp, k, np.bincount(comp, minlength=k)


def _scene_on_disk(tmp_path):
    from test_gpu_mesh_metrics import _write_eval
    scene, labels, sd = _blob_scene()[:3]
    _write_eval(tmp_path, scene)
    pred = torch.from_numpy(np.stack([-sd, sd], 1).astype(np.float32)).to(DEV)
    assert np.array_equal(pred.argmax(1).cpu().numpy(), labels)
    data = Config(path=str(tmp_path), gtfile="gt/0", filename="0", id="m", category="", infinite=torch.zeros(len(labels), dtype=torch.int32))
    return data, pred


def _clf(metrics, components=None, evaluation=False):
    clf = Config(temp=Config(graph_cut=0, fix_orientation=1, metrics=list(metrics), device=DEV), mesh=Config(solver="gpu"))
    if components is not None:
        clf.mesh.components = components
    if evaluation:
        clf.evaluation = Config(solver="gpu", seed=0)
    return clf


def test_generate_reports_the_components_of_an_unfiltered_mesh(tmp_path, capsys):
    from dgnn_amd.processing.generate_mesh import generate, mesh_components_gpu
    _, _, _, _, faces, _, k, _ = _blob_scene()
    data, pred = _scene_on_disk(tmp_path)
    mesh, ev = generate(data, pred, _clf(["watertight", "components"]))
    assert np.array_equal(mesh.vertex_ids[mesh.faces], faces)                    # today's mesh
    assert ev == {"watertight": mt.topology(mt.compact(faces)[0])["watertight"], "components": k}
    assert mesh_components_gpu(mesh) == k and mesh.n_removed_faces == 0
    mesh0, ev0 = generate(data, pred, _clf(["watertight"]))                      # without the metric: today's dict
    assert set(ev0) == {"watertight"} and np.array_equal(mesh0.faces, mesh.faces) and np.array_equal(mesh0.vertices, mesh.vertices)
    assert "WARNING" not in capsys.readouterr().out


@pytest.mark.parametrize("rule", ["largest", "min_faces"])
def test_generate_drops_the_small_components(tmp_path, capsys, rule):
    from dgnn_amd.processing.generate_mesh import chamfer_gpu, generate, iou_mesh_gpu
    scene, _, _, ids, faces, comp, k, counts = _blob_scene()
    data, pred = _scene_on_disk(tmp_path)
    value = "largest" if rule == "largest" else int(np.sort(counts)[-2]) + 1      # more faces than the second largest component has
    keep = mc.keep_mask(comp, counts, largest=True)
    if rule == "min_faces":
        assert np.array_equal(keep, mc.keep_mask(comp, counts, min_faces=value))
    clf = _clf(["watertight", "components", "iou", "chamfer"], components=value, evaluation=True)
    mesh, ev = generate(data, pred, clf)
    assert np.array_equal(mesh.vertex_ids[mesh.faces], faces[keep])
    assert mc.components(mesh.faces)[1] == 1 and ev["components"] == 1
    assert ev["n_removed_faces"] == mesh.n_removed_faces == int((~keep).sum()) > 0
    assert ev["watertight"] == mt.topology(mesh.faces)["watertight"]
    assert ev["iou"] == iou_mesh_gpu(data, mesh.vertices, mesh.faces, device=DEV) and 0 < ev["iou"] < 1
    assert ev["chamfer"] == chamfer_gpu(data, scene, torch.from_numpy(ids[keep]).to(DEV), clf) and np.isfinite(ev["chamfer"])
    _, ev_all = generate(data, pred, _clf(["iou", "chamfer"], evaluation=True))
    assert ev_all["chamfer"] != ev["chamfer"]                                      # the blob's facets are no longer sampled
    assert "WARNING" not in capsys.readouterr().out


def test_generate_keeps_the_mesh_when_a_device_step_of_the_filter_fails(tmp_path, capsys, monkeypatch):
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    from dgnn_amd.processing.generate_mesh import generate
    _, _, _, _, faces, _, k, _ = _blob_scene()
    data, pred = _scene_on_disk(tmp_path)
    real = ops.mesh_component_measures

    def measures_with_a_bad_count(vertices, faces_, comp, K):          # the library's own refusal: more components than faces
        return real(vertices, faces_, comp, len(faces_) + 1)
    monkeypatch.setattr(ops, "mesh_component_measures", measures_with_a_bad_count)
    with pytest.raises(DgnnError):
        measures_with_a_bad_count(mc.UNIT_TET, mc.unit_tet()[1], np.zeros(4, dtype=np.int32), 1)
    mesh, ev = generate(data, pred, _clf(["components"], components="largest"))
    assert "WARNING: Could not filter the components of mesh 0" in capsys.readouterr().out
    assert np.array_equal(mesh.vertex_ids[mesh.faces], faces) and ev == {"n_removed_faces": 0, "components": k}


@pytest.mark.parametrize("value", ["biggest", 0, -3, True, 2.5])
def test_generate_refuses_a_mistyped_components_key(tmp_path, value):
    from dgnn_amd.processing.generate_mesh import generate
    data, pred = _scene_on_disk(tmp_path)
    with pytest.raises(ValueError, match="mesh.components"):
        generate(data, pred, _clf(["components"], components=value))


def test_evaluate_reports_the_topology_of_a_foreign_mesh():
    from dgnn_amd.processing.evaluate_mesh import evaluate
    v, f, _, k, m = _case("shells")
    assert evaluate(v, f, topology=True) == {"components": 5, "largest_component_faces": 4, "watertight": 0}
    v, f = mc.unit_tet()
    assert evaluate(v, f, topology=True) == {"components": 1, "largest_component_faces": 4, "watertight": 1}
    assert evaluate(v, f[:0], topology=True) == {"components": 0, "largest_component_faces": 0, "watertight": 0}
    assert evaluate(v, f) == {}
