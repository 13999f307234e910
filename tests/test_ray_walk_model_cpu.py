"""The rule of the facet-ray walk (tests/ray_walk_model.py) on the CPU: in general position the walk visits exactly the cells
an all-pairs segment / tet test finds and starts where the vertex family starts; on Kuhn grids, where rays run along edges, through
vertices and inside facets, the symbolic perturbation gets every ray through (a condition of the rule, not a measurement)."""
import numpy as np
import pytest

import ray_walk_model as rw
import scene_features_model as sf


def test_general_position_the_walk_visits_the_all_pairs_cells_and_starts_where_the_vertex_family_does():
    v, tets, nbr, rv, s, kw, out = rw.case("general")
    assert len(v) == 150 and len(rv) == 150
    st = out["stats"]
    assert st["perturbed"] == 0 and st["stuck"] == 0 and st["capped"] == 0 and st["depth"] == 0 and st["used"] == 150
    started = out["ray_start"] >= 0
    assert np.isin(out["ray_status"][started], (rw.SENSOR, rw.HULL)).all() and (out["ray_status"][~started] == rw.NONE).all()
    assert st["sensor"] > 20 and st["hull"] > 100 and out["ray_starts"].max() == 1
    vr = sf.vertex_rays(v, tets, rv, s)
    assert np.array_equal(out["ray_start"], vr["ray_tet"])
    for r in range(len(rv)):
        for side in (rw.OUTSIDE, rw.INSIDE):
            walked = rw.walked_cells(out, r, side)
            assert len(set(walked)) == len(walked)
            assert set(walked) == rw.crossed_cells(v, tets, v[rv[r]], s[r], side), (r, side)


def test_general_position_distances_ascend_along_a_ray_and_chain_from_cell_to_cell():
    v, tets, nbr, rv, s, kw, out = rw.case("general")
    rec = out["records"]
    vr = sf.vertex_rays(v, tets, rv, s)
    assert (rec["first"] < rec["second"]).all() and (rec["first"] > 0).all()
    same = (rec["ray"][1:] == rec["ray"][:-1]) & (rec["side"][1:] == rec["side"][:-1])
    assert np.array_equal(rec["first"][1:][same], rec["second"][:-1][same]) and (rec["step"][1:][same] == rec["step"][:-1][same] + 1).all()
    head = rec["step"] == 0          # the first recorded cell is entered where the vertex family's cell is left
    assert np.array_equal(rec["first"][head], vr["ray_dist"][rec["ray"][head], rec["side"][head]])
    ends = np.r_[~same, True] & (rec["side"] == rw.OUTSIDE) & (out["ray_status"][rec["ray"], 0] == rw.SENSOR)
    assert np.array_equal(rec["second"][ends], np.sqrt((((s - v[rv]) ** 2)[:, 0] + ((s - v[rv]) ** 2)[:, 1]) + ((s - v[rv]) ** 2)[:, 2])[rec["ray"][ends]])
    assert (rec["slot"][ends] == -1).all() and (rec["slot"][~ends] >= 0).all()


@pytest.mark.parametrize("m", [3, 4, 5])
def test_kuhn_grids_no_ray_is_stuck_and_no_ray_has_two_start_cells(m):
    v, tets, nbr, rv, s, kw, out = rw.case("kuhn%d" % m)
    assert sf.cell_geometry(v, tets)["n_flat"] == 0 and len(tets) == 6 * (m - 1) ** 3
    st = out["stats"]
    print(m, st)
    assert st["stuck"] == 0 and st["capped"] == 0 and out["ray_starts"].max() <= 1
    assert st["perturbed"] > st["used"] // 2 and st["exact_used"] > 0 and st["sensor"] > 0 and st["hull"] > 0
    assert st["used"] + st["skipped"] == len(rv) and st["records"] == int(out["ray_cells"].sum())


def test_the_naive_tie_rule_is_not_enough_on_a_kuhn_grid(monkeypatch):
    """without the axis terms (a zero sign stays zero) rays that run inside facets and along edges do not get through"""
    v, tets, nbr, rv, s, kw, _ = rw.case("kuhn4")
    monkeypatch.setattr(rw._Ray, "sigma", lambda self, a, b: self.orient(self.p, self.s, a, b))
    out = rw.ray_walk(v, tets, nbr, rv, s, **kw)
    assert out["stats"]["stuck"] > 0 or out["ray_starts"].max() > 1


def test_depth_limits_cut_a_walk_short_and_change_nothing_before_the_cut():
    v, tets, nbr, rv, s, kw, full = rw.case("general")
    out = rw.ray_walk(v, tets, nbr, rv, s, unique=True, outside_depth=2, inside_depth=1)
    assert np.array_equal(out["ray_cells"], np.minimum(full["ray_cells"], [2, 1]))
    cut = full["ray_cells"] > [2, 1]
    assert (out["ray_status"][cut] == rw.DEPTH).all() and cut.any()
    # a walk that ends on its own in exactly `depth` cells keeps its status unless the depth came first: the hull is seen after the record
    short = full["ray_cells"] < [2, 1]
    assert np.array_equal(out["ray_status"][short], full["ray_status"][short])
    fr, orc = full["records"], out["records"]
    keep = fr["step"] < np.array([2, 1])[fr["side"]]
    for k in rw.RECORD_KEYS:
        if k != "second" and k != "slot":
            assert np.array_equal(fr[k][keep], orc[k]), k
    assert out["stats"]["records"] == int(keep.sum())


def test_a_ray_to_its_own_vertex_is_skipped_and_unique_keeps_the_lowest_ray_of_a_vertex():
    v, tets, nbr, rv, s, kw, out = rw.case("one_tet")
    assert out["stats"]["skipped"] == 1 and out["stats"]["used"] == 4 and (out["ray_status"][4] == rw.NONE).all()
    assert out["ray_status"][:4, 0].tolist() == [rw.HULL, rw.SENSOR, rw.SENSOR, rw.NONE] and out["stats"]["records"] == 0
    u = rw.ray_walk(v, tets, nbr, rv, s, unique=True, outside_depth=0, inside_depth=0)
    assert u["stats"]["skipped"] == 2 and u["ray_status"][2].tolist() == [rw.NONE, rw.NONE] and u["ray_status"][1, 0] == rw.SENSOR
    v, tets, nbr, rv, s, kw, out = rw.case("two_tets")
    # the rays through the edge (1, 2) and through vertex 1 run inside hull facets: the perturbed line passes outside the hull, no cell starts them
    assert out["ray_status"][:, 0].tolist() == [rw.HULL, rw.NONE, rw.SENSOR, rw.NONE, rw.SENSOR, rw.SENSOR] and out["stats"]["stuck"] == 0
    assert out["ray_cells"][:, 0].tolist() == [1, 0, 1, 0, 1, 0] and out["stats"]["perturbed"] == 5 and out["records"]["slot"].tolist() == [0, -1, -1]
    u = rw.ray_walk(v, tets, nbr, rv, s, unique=True, outside_depth=0, inside_depth=0)
    assert u["stats"]["used"] == 2 and u["stats"]["skipped"] == 4


def test_the_aggregates_are_the_fold_of_the_records():
    v, tets, nbr, rv, s, kw, out = rw.case("count_65")
    rec = out["records"]
    for side, name in enumerate(rw.SIDES):
        sel = rec["side"] == side
        assert np.array_equal(out[name + "_cell_count"], np.bincount(rec["cell"][sel], minlength=len(tets)))
        hit = sel & (rec["slot"] >= 0)
        assert np.array_equal(out[name + "_slot_count"].reshape(-1), np.bincount(4 * rec["cell"][hit] + rec["slot"][hit], minlength=4 * len(tets)))
        c = int(np.argmax(out[name + "_cell_count"]))
        assert out[name + "_cell_count"][c] > 1 and out[name + "_cell_second_max"][c] == rec["second"][sel & (rec["cell"] == c)].max()
        assert out[name + "_cell_first_min"][c] == rec["first"][sel & (rec["cell"] == c)].min()
