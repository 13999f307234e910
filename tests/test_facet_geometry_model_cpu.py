"""The CPU model of the `_fgeom` columns (tests/facet_geometry_model.py) against closed forms, its own symmetries, the graph-cut
weights' model on the facets they share, and its extended-precision evaluation; and the library's new entry points."""
import os

import numpy as np
import pytest

import facet_geometry_model as fgm
import graph_cut_weights_model as gwm
import mesh_metrics_model as mmm
import scene_features_model as sf

KEYS = fgm.FGEOM_KEYS
# the fp64 / longdouble distance of §23's construction was reported as 3e-15, 1.3e-14 and 1.1e-13 on 525 / 4 813 / 25 789 facets:
# the scenes here are smaller than the largest of them
LONGDOUBLE = 1.1e-13
FEW_ULP = 4          # the closed forms hold "to a few ulp" of their value


def _close(got, want):
    want = np.asarray(want, dtype=np.float64)
    return bool((np.abs(np.asarray(got) - want) <= FEW_ULP * np.spacing(np.abs(want))).all())


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _check_ranges(g):
    for k in KEYS:
        assert np.isfinite(g[k]).all(), k
    assert (np.abs(g["cos_own"]) <= 1).all() and (np.abs(g["cos_neighbor"]) <= 1).all() and (g["beta"] >= 0).all() and (g["beta"] <= 2).all()
    assert (g["area"] >= 0).all()


def test_closed_forms_of_the_two_cell_scenes():
    s = gwm.regular_pair_scene()
    g = fgm.facet_geometry(s)
    r0, r1 = fgm.facet_rows(s)[0]
    for r in (r0, r1):
        assert _close(g["cos_own"][r], 1 / 3) and _close(g["cos_neighbor"][r], 1 / 3) and _close(g["beta"][r], 2 / 3)
        assert _close(g["area"][r], np.sqrt(3.0) / 4)
    assert g["stats"] == dict(rows=8, hull_rows=6, neutral_sides=0, n_flat=0) and (g["written"] == 1).all()
    for face, want in (("z0", 1 / np.sqrt(3.0)), ("diag", -1.0 / 3.0)):
        s = gwm.corner_scene(face)
        g = fgm.facet_geometry(s)
        _check_ranges(g)
        rows = fgm.facet_rows(s)
        for r in rows[0]:
            assert _close(g["cos_own"][r], want) and _close(g["cos_neighbor"][r], want) and _close(g["beta"][r], 1 - want)
        hull = rows[1:, 0]
        assert (rows[1:, 1] < 0).all() and len(hull) == 6 == g["stats"]["hull_rows"]
        assert (g["cos_neighbor"][hull] == 1.0).all()
        assert np.array_equal(_bits(g["beta"][hull]), _bits(1.0 - g["cos_own"][hull]))


def test_a_single_tet_has_four_hull_rows():
    g = fgm.facet_geometry(fgm.single_tet_scene())
    assert g["stats"] == dict(rows=4, hull_rows=4, neutral_sides=0, n_flat=0) and (g["written"] == 1).all()
    # the corner cell: 1/sqrt(3) at its three faces through the origin, -1/3 at x + y + z = 1 (slot 0)
    assert _close(g["cos_own"][0], -1 / 3) and _close(g["cos_own"][1:], np.full(3, 1 / np.sqrt(3.0)))
    assert (g["cos_neighbor"] == 1.0).all() and np.array_equal(_bits(g["beta"]), _bits(1.0 - g["cos_own"]))
    assert _close(g["area"], [np.sqrt(3.0) / 2, 0.5, 0.5, 0.5])


def test_degenerate_sides_are_neutral_and_counted_and_everything_is_finite():
    s = gwm.degenerate_scene()
    g = fgm.facet_geometry(s)
    _check_ranges(g)
    # the four neutral sides of §23's count (the flat cell 1 at facets 0 and 1, both sides of the facet without area); cells 1, 3 and 4 are flat
    assert g["stats"] == dict(rows=8, hull_rows=2, neutral_sides=4, n_flat=3)
    rows = fgm.facet_rows(s)
    assert g["cos_own"][rows[0, 1]] == 0 and g["cos_neighbor"][rows[0, 0]] == 0 and g["cos_own"][rows[1, 0]] == 0          # cell 1's sides
    for r in rows[2]:                                                                                                        # the facet 6-7-8
        assert g["area"][r] == 0 and g["cos_own"][r] == 0 and g["cos_neighbor"][r] == 0 and g["beta"][r] == 1.0
    sph = fgm.cell_circumspheres(s["vertices"], s["tetrahedra"])
    assert sph["n_flat"] == 3 and not np.isfinite(sph["radius"][[1, 3, 4]]).any() and np.isfinite(sph["radius"][[0, 2]]).all()


def test_circumspheres_pass_through_the_four_vertices():
    s = mmm.random_scene(40, 1)
    sph = fgm.cell_circumspheres(s["vertices"], s["tetrahedra"])
    d = np.linalg.norm(s["vertices"][s["tetrahedra"]] - sph["centre"][:, None, :], axis=2)
    assert sph["n_flat"] == 0 and (np.abs(d - sph["radius"][:, None]) <= 1e-9 * sph["radius"][:, None]).all()


@pytest.fixture(scope="module", params=[(5, 3), (40, 1), (300, 2)], ids=lambda p: "%dpts" % p[0])
def scene(request):
    return mmm.random_scene(*request.param)


def test_every_row_is_written_once_and_the_two_rows_of_a_facet_mirror_each_other(scene):
    g = fgm.facet_geometry(scene)
    _check_ranges(g)
    t = len(scene["tetrahedra"])
    assert g["stats"]["rows"] == 4 * t and (g["written"] == 1).all() and g["stats"]["neutral_sides"] == 0 and g["stats"]["n_flat"] == 0
    nbr, bad = sf.tet_neighbors(scene["facets"], scene["nfacets"], scene["tetrahedra"])
    assert bad == 0 and g["stats"]["hull_rows"] == int((nbr < 0).sum())
    c, k = np.nonzero(nbr >= 0)
    n = nbr[c, k].astype(np.int64)
    back = np.argmax(nbr[n] == c[:, None], axis=1)
    assert (nbr[n, back] == c).all()
    row, mirror = 4 * c + k, 4 * n + back
    for a, b in (("area", "area"), ("beta", "beta"), ("cos_own", "cos_neighbor"), ("cos_neighbor", "cos_own")):
        assert np.array_equal(_bits(g[a][row]), _bits(g[b][mirror])), (a, b)
    hull = np.nonzero((nbr < 0).reshape(-1))[0]
    assert (g["cos_neighbor"][hull] == 1.0).all() and np.array_equal(_bits(g["beta"][hull]), _bits(1.0 - g["cos_own"][hull]))


def test_beta_is_the_graph_cut_term_at_finite_finite_facets(scene):
    g = fgm.facet_geometry(scene)
    q = gwm.facet_terms(scene, "beta")
    rows = fgm.facet_rows(scene)
    both = gwm.graph_rows(scene["nfacets"])
    assert both.any()
    for s in (0, 1):
        assert np.array_equal(_bits(g["beta"][rows[both, s]]), _bits(q[both]))


def test_fp64_columns_are_their_longdouble_evaluation_to_rounding(scene):
    g64, gld = fgm.facet_geometry(scene), fgm.facet_geometry(scene, np.longdouble)
    assert g64["stats"] == gld["stats"]
    for k in KEYS:
        d = float(np.abs(g64[k] - gld[k]).max())
        print("%s: %d rows, max |fp64 - longdouble| = %.3g" % (k, len(g64[k]), d))
        assert d <= LONGDOUBLE, k


def test_the_order_of_the_facets_and_of_their_two_sides_does_not_matter(scene):
    g = fgm.facet_geometry(scene)
    rng = np.random.default_rng(7)
    perm = rng.permutation(len(scene["facets"]))
    nf = scene["nfacets"][perm].copy()
    swap = rng.random(len(nf)) < 0.5
    nf[swap] = nf[swap][:, ::-1]
    h = fgm.facet_geometry(dict(scene, facets=scene["facets"][perm], nfacets=nf))
    assert h["stats"] == g["stats"] and swap.any() and not swap.all()
    for k in KEYS:
        assert np.array_equal(_bits(g[k]), _bits(h[k])), k


def test_malformed_scenes_raise():
    s = gwm.regular_pair_scene()
    for key, at, value in (("facets", (0, 1), 99), ("nfacets", (0, 1), 2), ("tetrahedra", (1, 3), 7)):
        bad = dict(s, **{key: s[key].copy()})
        bad[key][at] = value
        with pytest.raises(gwm.MalformedScene):
            fgm.facet_geometry(bad)
    bad = dict(s, nfacets=s["nfacets"].copy())
    bad["nfacets"][1] = [0, 1]               # a hull facet of cell 0 said to border cell 1 as well
    with pytest.raises(gwm.MalformedScene):
        fgm.facet_geometry(bad)


def test_library_exports_the_facet_geometry():
    import ctypes
    from dgnn_amd._lib import LIB_PATH, SIGNATURES
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    raw = ctypes.CDLL(LIB_PATH)
    for name in ("dgnn_cell_circumspheres", "dgnn_cell_circumspheres_scratch_bytes", "dgnn_facet_geometry", "dgnn_facet_geometry_scratch_bytes"):
        assert hasattr(raw, name) and name in SIGNATURES, name
    fn = raw.dgnn_facet_geometry_scratch_bytes
    fn.restype, fn.argtypes = SIGNATURES["dgnn_facet_geometry_scratch_bytes"]
    assert fn(1000) >= 32 * 1000 + 256 and fn(-1) == 0
    from dgnn_amd import ops
    from dgnn_amd.processing import scene_features
    assert ops.FGEOM_KEYS == scene_features.FGEOM_KEYS == fgm.FGEOM_KEYS == ("area", "cos_own", "cos_neighbor", "beta")
