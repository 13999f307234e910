"""The `_fgeom` columns on the device (ops.cell_circumspheres / ops.facet_geometry) against the CPU model
(tests/facet_geometry_model.py) bit for bit, against ops.facet_cut_terms on the facets both weigh, and their behaviour on bad data."""
import functools

import numpy as np
import pytest
import torch

import facet_geometry_model as fgm
import graph_cut_weights_model as gwm
import mesh_metrics_model as mmm
from helpers import gold

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = fgm.FGEOM_KEYS
RANDOM = {"5pts": (5, 3), "40pts": (40, 1), "300pts": (300, 2)}


def _bits(x):
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _ignatius():
    """the finite cells of Ignatius with every facet listed once by its lower cell (the fixture holds vertices and tetrahedra only)"""
    import scene_features_model as sf
    g = gold("ignatius_3dt.npz")
    fx = sf.load_fixture()
    return dict(vertices=np.asarray(g["vertices"], dtype=np.float64), tetrahedra=np.asarray(g["tetrahedra"], dtype=np.int32),
                facets=np.asarray(fx["facets"], dtype=np.int32), nfacets=np.asarray(fx["nfacets"], dtype=np.int32))


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(scene, the model's columns and stats, the model's spheres); read only"""
    if name in RANDOM:
        s = mmm.random_scene(*RANDOM[name])
    elif name == "ignatius":
        s = _ignatius()
    else:
        s = {"single": fgm.single_tet_scene, "regular": gwm.regular_pair_scene, "corner_z0": lambda: gwm.corner_scene("z0"),
             "corner_diag": lambda: gwm.corner_scene("diag"), "degenerate": gwm.degenerate_scene}[name]()
    return s, fgm.facet_geometry(s), fgm.cell_circumspheres(s["vertices"], s["tetrahedra"])


def _run(s, **kw):
    from dgnn_amd import ops
    return ops.facet_geometry(s["vertices"], s["tetrahedra"], s["facets"], s["nfacets"], **kw)


NAMES = ["single", "regular", "corner_z0", "corner_diag", "degenerate", "5pts", "40pts", "300pts", "ignatius"]


def test_the_random_scenes_straddle_one_block_and_no_tet_count_fills_its_waves():
    f = {k: len(_scene(k)[0]["facets"]) for k in RANDOM}
    t = {k: len(_scene(k)[0]["tetrahedra"]) for k in RANDOM}
    print(f, t)
    assert f["5pts"] < 256 < f["300pts"] and all(v % 64 for v in t.values())
    ig = _scene("ignatius")[0]
    assert len(ig["tetrahedra"]) == 66685 and len(ig["facets"]) == (4 * 66685 + 332) // 2 == 133536          # 332 hull facets: the grid-stride loop


@pytest.mark.parametrize("name", NAMES)
def test_columns_and_stats_are_the_models_bit_for_bit(name):
    s, want, _ = _scene(name)
    got = _run(s)
    assert sorted(got) == sorted(KEYS + ("stats",))
    for k in KEYS:
        assert got[k].is_cuda and got[k].dtype == torch.float64 and tuple(got[k].shape) == (4 * len(s["tetrahedra"]),), k
        assert np.array_equal(_bits(got[k]), _bits(want[k])), "%s: max |d| = %g" % (k, np.abs(got[k].cpu().numpy() - want[k]).max())
        assert bool(torch.isfinite(got[k]).all()), k
    assert got["stats"] == want["stats"]
    if name == "ignatius":
        assert want["stats"]["rows"] == 4 * 66685 and want["stats"]["hull_rows"] > 0 and (want["written"] == 1).all()
    if name == "single":
        assert got["stats"]["rows"] == 4 and got["stats"]["hull_rows"] == 4
    if name == "degenerate":
        assert got["stats"]["neutral_sides"] == 4 and got["stats"]["n_flat"] == 3


@pytest.mark.parametrize("name", NAMES)
def test_circumspheres_are_the_models_bit_for_bit_and_can_be_handed_on(name):
    from dgnn_amd import ops
    s, want, sph = _scene(name)
    got = ops.cell_circumspheres(s["vertices"], s["tetrahedra"])
    t = len(s["tetrahedra"])
    assert got["centre"].is_cuda and tuple(got["centre"].shape) == (t, 3) and tuple(got["radius"].shape) == (t,) and got["radius"].dtype == torch.float64
    assert np.array_equal(_bits(got["centre"]), _bits(sph["centre"])) and np.array_equal(_bits(got["radius"]), _bits(sph["radius"]))
    assert got["n_flat"] == sph["n_flat"] == want["stats"]["n_flat"]
    again = _run(s, spheres=got)          # the facet pass alone, from the stored records
    assert again["stats"] == want["stats"] and all(np.array_equal(_bits(again[k]), _bits(want[k])) for k in KEYS)
    if name == "300pts":
        # records that start 8 bytes into a larger tensor are copied, not refused; a dict that is not cell_circumspheres' is refused by name
        shifted = torch.zeros(4 * t + 1, dtype=torch.float64, device=DEV)
        shifted[1:] = got["records"].reshape(-1)
        view = _run(s, spheres=dict(records=shifted[1:].view(t, 4), n_flat=got["n_flat"]))
        assert view["stats"] == want["stats"] and all(np.array_equal(_bits(view[k]), _bits(want[k])) for k in KEYS)
        for bad in (dict(centre=got["centre"], radius=got["radius"]), dict(records=got["records"][:-1], n_flat=0)):
            with pytest.raises(ValueError):
                _run(s, spheres=bad)


@pytest.mark.parametrize("name", ["ignatius", "300pts", "degenerate"])
def test_beta_is_the_cut_terms_q_at_finite_finite_facets(name):
    """the recompute form of cutterms.hip and the two-pass form here share csrc/facet_geom.h: one meaning, the same bits"""
    from dgnn_amd import ops
    s, want, _ = _scene(name)
    _, q, st = ops.facet_cut_terms(s["vertices"], s["tetrahedra"], s["facets"], s["nfacets"], "beta", 10, return_q=True)
    q = q.cpu().numpy()
    both = gwm.graph_rows(s["nfacets"])
    rows = fgm.facet_rows(s)
    beta = _run(s)["beta"].cpu().numpy()
    assert both.any() and st["rows"] == int(both.sum())
    for side in (0, 1):
        assert np.array_equal(_bits(beta[rows[both, side]]), _bits(q[both]))


def test_facet_order_and_side_order_do_not_matter_and_reruns_are_identical():
    s, want, _ = _scene("300pts")
    rng = np.random.default_rng(7)
    perm = rng.permutation(len(s["facets"]))
    nf = s["nfacets"][perm].copy()
    swap = rng.random(len(nf)) < 0.5
    nf[swap] = nf[swap][:, ::-1]
    a, b, c = _run(s), _run(dict(s, facets=s["facets"][perm], nfacets=nf)), _run(s)
    assert a["stats"] == b["stats"] == c["stats"]
    for k in KEYS:
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) and torch.equal(a[k].view(torch.int64), c[k].view(torch.int64)), k


def test_outputs_live_on_the_inputs_device():
    from dgnn_amd import ops
    s, want, _ = _scene("40pts")
    dev = torch.device("cuda", torch.cuda.device_count() - 1)
    t = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
    got = ops.facet_geometry(t["vertices"], t["tetrahedra"], t["facets"], t["nfacets"])
    sph = ops.cell_circumspheres(t["vertices"], t["tetrahedra"])
    assert all(got[k].device == dev for k in KEYS) and sph["centre"].device == dev and sph["radius"].device == dev
    assert all(np.array_equal(_bits(got[k]), _bits(want[k])) for k in KEYS)


def test_bad_data_is_refused_by_a_check():
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    s = gwm.regular_pair_scene()
    bad = dict(s, facets=s["facets"].copy())
    bad["facets"][0, 1] = 99                                          # a facet's vertex id out of range
    with pytest.raises(DgnnError, match="out of range"):
        _run(bad)
    bad["facets"][0, 1] = -1
    with pytest.raises(DgnnError, match="out of range"):
        _run(bad)
    bad = dict(s, tetrahedra=s["tetrahedra"].copy())
    bad["tetrahedra"][1, 3] = 1 << 30                                 # a cell's vertex id out of range
    with pytest.raises(DgnnError, match="out of range"):
        _run(bad)
    with pytest.raises(DgnnError, match="out of range"):
        ops.cell_circumspheres(bad["vertices"], bad["tetrahedra"])
    bad = dict(s, nfacets=s["nfacets"].copy())
    bad["nfacets"][0, 1] = 2                                          # a cell id == T
    with pytest.raises(DgnnError, match="out of range"):
        _run(bad)
    bad = dict(s, nfacets=s["nfacets"].copy())
    bad["nfacets"][1] = [0, 1]                                        # a hull facet of cell 0 said to border cell 1 as well
    with pytest.raises(DgnnError, match="not a face"):
        _run(bad)
    with pytest.raises(ValueError):
        ops.facet_geometry(s["vertices"], s["tetrahedra"], s["facets"], s["nfacets"][:-1])
    # no cells, no facets; and a good call after the failed ones
    empty = ops.facet_geometry(s["vertices"], np.zeros((0, 4), np.int32), np.zeros((0, 3), np.int32), np.zeros((0, 2), np.int32))
    assert empty["stats"] == dict(rows=0, hull_rows=0, neutral_sides=0, n_flat=0) and empty["area"].numel() == 0
    assert _run(s)["stats"] == fgm.facet_geometry(s)["stats"]
