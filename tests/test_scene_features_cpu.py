"""The CPU model of the scene front end (tests/scene_features_model.py) against the files the reference's external binary recorded for
Ignatius scene 99 (tests/golden/ignatius_scene_features*.npz): the definitions of DESIGN §25 reproduce them -- counts and edge lengths
exactly, the distances and vol / radius to the last bits -- and the model's hand-made cases say what the tie rules mean."""
import functools
import os

import numpy as np

import scene_features_model as sf
from helpers import GOLD, gold


@functools.lru_cache(maxsize=None)
def ignatius():
    """-> (fixture dict, vertices, tetrahedra, infinite, adj_dst, recorded columns in full rows); read only"""
    fx = sf.load_fixture()
    g = gold("ignatius_3dt.npz")
    rec = sf.recorded_columns(fx)
    for a in rec.values():
        a.setflags(write=False)
    return fx, g["vertices"], g["tetrahedra"], g["infinite"], gold("static_f4_ignatius_full.npz")["adj_dst"], rec


@functools.lru_cache(maxsize=None)
def ignatius_model():
    fx, v, tets, inf, _, _ = ignatius()
    vid = sf.match_vertices(v, fx["points"])
    assert (vid >= 0).all()
    geom = sf.cell_geometry(v, tets)
    rays = sf.vertex_rays(v, tets, vid, fx["sensor_position"])
    return geom, rays, sf.scene_columns(geom, rays, inf)


def test_fixture_parts_stay_below_the_size_limit():
    parts = [f for f in os.listdir(GOLD) if f.startswith(sf.FIXTURE_STEM) and f.endswith(".npz")]
    assert len(parts) >= 1 and all(os.path.getsize(os.path.join(GOLD, f)) < 1024 * 1024 for f in parts)
    assert sum(os.path.getsize(os.path.join(GOLD, f)) for f in parts) < 4_000_000


def test_model_reproduces_the_recorded_cell_geometry_and_vertex_ray_files():
    geom, rays, cols = ignatius_model()
    _, _, _, inf, _, rec = ignatius()
    sf.check_against_recorded(cols, rec)
    assert rays["stats"]["no_outside"] == 159 and rays["stats"]["no_inside"] == 49 and rays["stats"]["duplicates"] == 7
    assert geom["n_flat"] == 0
    want = (rec["longest_edge"].sum() + rec["shortest_edge"].sum()) / (2 * len(inf))          # processing/data.py, numpy's pairwise sum
    assert abs(sf.mean_edge(geom, len(inf)) - want) <= 1e-13 * want


def test_either_ray_of_a_duplicate_pair_gives_the_recorded_files():
    fx, v, tets, inf, _, rec = ignatius()
    vid = sf.match_vertices(v, fx["points"])
    geom, _, _ = ignatius_model()
    rev = np.arange(len(vid))[::-1]          # the last ray of every vertex becomes its lowest index
    rays = sf.vertex_rays(v, tets, vid[rev], fx["sensor_position"][rev])
    sf.check_against_recorded(sf.scene_columns(geom, rays, inf), rec)


def test_model_neighbors_are_the_recorded_adjacency():
    fx, _, tets, inf, adj_dst, _ = ignatius()
    nbr, bad = sf.tet_neighbors(fx["facets"], fx["nfacets"], tets)
    assert bad == 0
    cell_of_tet, tet_of_cell = sf.cell_rows(inf)
    dst = adj_dst.reshape(-1, 4)[cell_of_tet]                       # row 4 c + k: the neighbour of cell c across the facet opposite vertex k
    both = nbr >= 0
    assert np.array_equal(tet_of_cell[dst][both], nbr[both])
    assert (np.asarray(inf)[dst[~both]] == 1).all() and (tet_of_cell[dst][both] >= 0).all()


def test_a_facet_that_is_no_face_of_its_cell_is_counted():
    tets = np.array([[0, 1, 2, 3], [1, 2, 3, 4]])
    nbr, bad = sf.tet_neighbors(np.array([[1, 2, 3], [0, 1, 4]]), np.array([[0, 1], [0, -1]]), tets)
    assert bad == 1 and nbr.tolist() == [[1, -1, -1, -1], [-1, -1, -1, 0]]


def test_one_tet_rays_through_it_and_mirrored():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    tets = np.array([[0, 1, 2, 3]])
    centre = v.mean(axis=0)
    r = sf.vertex_rays(v, tets, np.arange(4), np.tile(centre, (4, 1)))
    assert r["ray_tet"].tolist() == [[0, -1]] * 4 and r["ray_slot"][:, 0].tolist() == [0, 1, 2, 3]
    assert r["outside_tet_count"].tolist() == [4] and r["outside_slot_count"].tolist() == [[1, 1, 1, 1]] and not r["inside_tet_count"].any()
    # from the origin towards the centroid the ray meets x + y + z = 1 at the centroid's direction: |(1/3, 1/3, 1/3)| = 1 / sqrt(3)
    assert abs(r["ray_dist"][0, 0] - 1 / np.sqrt(3)) < 1e-15
    m = sf.vertex_rays(v, tets, np.arange(4), 2 * v - centre)          # the sensors mirrored at their vertices
    assert m["ray_tet"].tolist() == [[-1, 0]] * 4 and np.array_equal(m["ray_dist"][:, 1], r["ray_dist"][:, 0])
    assert m["stats"]["no_outside"] == 4 and r["stats"]["no_inside"] == 4


def test_a_ray_in_a_shared_facet_takes_the_lower_tet_and_duplicates_follow_unique():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1]])
    tets = np.array([[0, 1, 2, 3], [0, 2, 1, 4]])                          # they share the facet (0, 1, 2) in the plane z = 0
    s = np.array([[0.25, 0.25, 0.0]])
    r = sf.vertex_rays(v, tets, [0], s)
    assert r["ray_tet"].tolist() == [[0, -1]] and abs(r["ray_dist"][0, 0] - np.sqrt(0.5)) < 1e-15
    r = sf.vertex_rays(v, tets[::-1], [0], s)
    assert r["ray_tet"].tolist() == [[0, -1]] and r["ray_slot"][0, 0] == 0          # the lower index, whichever tet carries it
    rv, ss = [0, 0, 0, 3], np.array([[0.25, 0.25, 0.0], [0.2, 0.2, 0.2], [0.0, 0, 0], [0, 0, 1.0]])
    u = sf.vertex_rays(v, tets, rv, ss)
    assert u["stats"] == dict(rays=4, used=1, duplicates=1, degenerate=2, no_outside=0, no_inside=1, exact_used=u["stats"]["exact_used"])
    a = sf.vertex_rays(v, tets, rv, ss, unique=False)
    assert a["stats"]["used"] == 2 and a["outside_tet_count"].tolist() == [2, 0] and a["outside_tet_sum"][0] == a["ray_dist"][0, 0] + a["ray_dist"][1, 0]
