"""ops.ray_walk (csrc/raywalk.hip) against the CPU model tests/ray_walk_model.py: the record stream, every aggregate bit for bit (the same
fp64 operations in the same order, the fold in ascending (ray, step)), status, counts and stats; the same bits for every max_records, on a
rerun and for any row order of the incidence.  No ray of any case may end stuck or capped."""
import inspect
import os

import numpy as np
import pytest
import torch

import ray_walk_model as rw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AGGREGATES = ["%s_%s" % (side, k) for side in rw.SIDES for k in
              ("cell_count", "slot_count", "cell_first_min", "cell_first_max", "cell_first_sum", "cell_second_min", "cell_second_max", "cell_second_sum",
               "slot_min", "slot_max", "slot_sum")]


def _t(x, dev=DEV):
    return torch.from_numpy(np.array(x)).to(dev)          # (a copy: the shared cases are read-only)


def _walk(which, dev=DEV, **over):
    from dgnn_amd import ops
    v, tets, nbr, rv, s, kw = rw.case(which)[:6]
    return ops.ray_walk(_t(v, dev), _t(tets, dev), _t(nbr, dev), _t(rv, dev), _t(s, dev), **dict(kw, **over))


def _same(a, b):
    """equal bits: fp64 compared as integers"""
    a, b = (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    if a.dtype == np.float64:
        return b.dtype == np.float64 and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))
    return a.dtype == b.dtype and np.array_equal(a, b)


def _assert_equal(got, want, records=True):
    assert got["stats"] == {k: want["stats"][k] for k in got["stats"]} and set(got["stats"]) == set(rw.STATS)
    assert _same(got["ray_status"], want["ray_status"]) and _same(got["ray_cells"], want["ray_cells"])
    for k in AGGREGATES:
        assert got[k].is_cuda and _same(got[k], want[k]), k
    if records:
        for k in rw.RECORD_KEYS:
            assert _same(got["records"][k], want["records"][k]), k


@pytest.mark.parametrize("which", rw.CASES)
def test_the_walk_equals_the_model_bit_for_bit(which):
    want = rw.case(which)[6]
    got = _walk(which, return_records=True)
    _assert_equal(got, want)
    assert got["stats"]["stuck"] == 0 and got["stats"]["capped"] == 0
    t = len(rw.case(which)[1])
    assert got["outside_cell_count"].shape == (t,) and got["inside_slot_sum"].shape == (t, 4) and got["ray_status"].shape == (len(rw.case(which)[3]), 2)


def test_the_cases_cover_what_they_are_meant_to():
    st = {c: rw.case(c)[6]["stats"] for c in rw.CASES}
    assert st["general"]["perturbed"] == 0 and st["general"]["sensor"] > 20 and st["general"]["hull"] > 100 and st["general"]["longest"] > 10
    assert st["general_scaled"]["records"] == st["general"]["records"]
    for m in (3, 4, 5):
        assert st["kuhn%d" % m]["perturbed"] > 0 and st["kuhn%d" % m]["exact_used"] > 100
    assert st["count_0"]["used"] == 0 and st["count_1"]["used"] == 1 and st["count_4097"]["used"] > 4000
    assert max(rw.case("count_4097")[6]["outside_cell_count"].max(), rw.case("count_4097")[6]["inside_cell_count"].max()) > 100   # long runs in the fold


@pytest.mark.parametrize("which", ["general", "kuhn4", "count_4097"])
def test_no_result_depends_on_max_records_and_a_rerun_gives_the_same_bits(which):
    want = rw.case(which)[6]
    longest = want["stats"]["longest"]
    assert longest >= 1
    base = _walk(which, return_records=True)
    for m in (longest, 7 * longest, None):
        got = _walk(which, max_records=m, return_records=True)
        _assert_equal(got, want)
        for k in AGGREGATES + ["ray_status", "ray_cells"]:
            assert _same(got[k], base[k]), (k, m)
        for k in rw.RECORD_KEYS:
            assert _same(got["records"][k], base["records"][k]), (k, m)


def test_depth_limits_and_unique_equal_the_model():
    from dgnn_amd import ops
    v, tets, nbr, rv, s = rw.case("general")[:5]
    want = rw.ray_walk(v, tets, nbr, rv, s)          # the defaults: every cell towards the sensor, one cell behind the surface
    got = ops.ray_walk(_t(v), _t(tets), _t(nbr), _t(rv), _t(s), return_records=True)
    _assert_equal(got, want)
    assert got["stats"]["depth"] > 0 and int(got["ray_cells"][:, 1].max()) == 1
    v, tets, nbr, rv, s = rw.case("kuhn3")[:5]
    want = rw.ray_walk(v, tets, nbr, rv, s, unique=True, outside_depth=2, inside_depth=3)
    got = ops.ray_walk(_t(v), _t(tets), _t(nbr), _t(rv), _t(s), unique=True, outside_depth=2, inside_depth=3, return_records=True)
    _assert_equal(got, want)
    assert got["stats"]["skipped"] >= 27


def test_a_prebuilt_incidence_in_any_row_order_gives_the_same_bits():
    from dgnn_amd import ops
    import scene_features_model as sf
    v, tets, nbr, rv, s, kw, want = rw.case("kuhn4")
    rowptr, entries = sf.vertex_incidence(tets, len(v))
    entries = entries.copy()
    rng = np.random.default_rng(0)
    for a, b in zip(rowptr[:-1], rowptr[1:]):
        entries[a:b] = rng.permutation(entries[a:b])
    got = ops.ray_walk(_t(v), _t(tets), _t(nbr), _t(rv), _t(s), incidence=(_t(rowptr), _t(entries)), return_records=True, **kw)
    _assert_equal(got, want)


def _with(a, index, value):
    c = np.array(a)
    c[index] = value
    return c


def test_bad_input_is_refused():
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    v, tets, nbr, rv, s, kw, want = rw.case("kuhn3")

    def walk(**o):
        return ops.ray_walk(*[_t(o.pop(k, x)) for k, x in (("v", v), ("tets", tets), ("nbr", nbr), ("rv", rv), ("s", s))], **dict(kw, **o))

    with pytest.raises(DgnnError):
        walk(rv=_with(rv, 0, len(v)))                          # no such vertex
    with pytest.raises(DgnnError):
        walk(tets=_with(tets, (0, 0), -1))
    with pytest.raises(DgnnError):
        walk(nbr=_with(nbr, (0, 0), len(tets)))                # no such cell
    with pytest.raises(DgnnError):
        walk(nbr=_with(nbr, (5, 1), -2))
    with pytest.raises(DgnnError):
        walk(s=_with(s, (3, 1), np.nan))
    with pytest.raises(DgnnError):
        walk(s=_with(s, (3, 1), 2.0 ** 301))                   # outside the exact predicate's range
    with pytest.raises(DgnnError):
        walk(v=_with(v, (2, 2), 2.0 ** -301))
    with pytest.raises(DgnnError):
        walk(max_records=want["stats"]["longest"] - 1)         # below the longest walk
    with pytest.raises(ValueError):
        walk(nbr=nbr[:-1])
    with pytest.raises(ValueError):
        walk(s=s[:-1])
    # a neighbour table that names, for a facet some ray leaves through, a cell that does not hold the facet: refused, not followed
    rec = want["records"]
    i = np.nonzero((rec["slot"] >= 0) & (nbr[rec["cell"], np.maximum(rec["slot"], 0)] >= 0))[0][0]
    c, k = int(rec["cell"][i]), int(rec["slot"][i])
    other = [t for t in range(len(tets)) if len(set(tets[t].tolist()) & set(tets[c].tolist())) < 3][0]
    with pytest.raises(DgnnError):
        walk(nbr=_with(nbr, (c, k), other))
    _assert_equal(_walk("kuhn3"), want, records=False)        # and the library works as before


@pytest.fixture
def current_device_calls(monkeypatch):
    """every call of torch.cuda.current_device() made from the package (the pattern of test_gpu_scene_features.py)"""
    real = torch.cuda.current_device
    calls = []

    def spy():
        caller = inspect.stack()[1].filename
        if os.sep + "dgnn_amd" + os.sep in caller:
            calls.append(caller)
        return real()
    monkeypatch.setattr(torch.cuda, "current_device", spy)
    return calls


def test_tensors_stay_on_the_device_of_the_inputs(current_device_calls):
    dev = torch.device("cuda", torch.cuda.device_count() - 1)          # a second device where there is one
    got = _walk("kuhn3", dev=dev, return_records=True)
    assert current_device_calls == []
    assert all(a.device == dev for k, a in got.items() if k not in ("stats", "records")) and all(a.device == dev for a in got["records"].values())
    _assert_equal(got, rw.case("kuhn3")[6])


@pytest.mark.parametrize("op", ["vertex_ray_features", "ray_walk"])
def test_both_ray_operations_refuse_the_same_bad_rays_and_differ_on_an_unused_vertex(op):
    """The checks the two operations share (csrc/tet_rays.h), on the six tets of one Kuhn cube (8 vertices), one ray per vertex.  Where they
    check differs on purpose: vertex_ray_features looks only at the coordinates a live ray reads, ray_walk at every vertex up front."""
    import scene_features_model as sf
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    v, tets, _ = rw.kuhn_grid(2)
    assert v.shape == (8, 3) and tets.shape == (6, 4)
    fac, nfac = sf.facets_from_tets(tets)
    nbr = ops.tet_neighbors(_t(fac), _t(nfac), _t(tets))
    rv, s = np.arange(8), 0.25 + 0.5 * v + np.array([0.03, 0.05, 0.07])          # sensors inside the cube, none at its vertex

    def run(vertices=v, ray_vertex=rv, sensors=s, **kw):
        args = (_t(vertices), _t(tets)) + ((nbr,) if op == "ray_walk" else ()) + (_t(ray_vertex), _t(sensors))
        return getattr(ops, op)(*args, **kw)

    assert run()["stats"]["used"] == 8
    nan_sensor, far_sensor = s.copy(), s.copy()
    nan_sensor[3, 1], far_sensor[5, 2] = np.nan, 2.0 ** 301
    rowptr, entries = sf.vertex_incidence(tets, 8)
    bad = [dict(ray_vertex=np.where(rv == 2, -1, rv)), dict(ray_vertex=np.where(rv == 6, 8, rv)), dict(sensors=nan_sensor), dict(sensors=far_sensor),
           dict(incidence=(_t(rowptr), _t(entries[::-1].copy())))]          # the last: rows that hold other vertices' corners
    for kw in bad:
        with pytest.raises(DgnnError):
            run(**kw)
    unused = np.concatenate([v, [[2.0 ** 301, 0.0, 0.0]]])          # a ninth vertex outside the predicate's range that no tet and no ray names
    if op == "ray_walk":
        with pytest.raises(DgnnError):
            run(vertices=unused)
    else:
        assert run(vertices=unused)["stats"]["used"] == 8
