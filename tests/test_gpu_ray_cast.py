"""ops.ray_first_hit (csrc/raycast.hip) against tests/ray_cast_model.py, which tests every (ray, face) pair without a grid: the
faces equal, t and the points bit for bit, the stats equal.  No tolerance anywhere."""
import functools
import inspect
import os

import numpy as np
import pytest
import torch

import mesh_contains_model as mc
import ray_cast_model as rc

pytestmark = pytest.mark.gpu
RESOLUTIONS = (1, 2, 7, 64, None)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "cube":
        return mc.cube(0.2, 0.8)
    if name == "int_cube":
        return mc.cube(0.0, 4.0)
    if name == "tetrahedron":
        return mc.tetrahedron()
    if name == "one_face":
        return np.array([[0.1, 0.2, 0.3], [0.9, 0.25, 0.4], [0.3, 0.8, 0.6], [np.nan, 0.0, 0.0]]), np.array([[0, 1, 2]], dtype=np.int32)
    if name == "shifted":          # the sphere at 2^-20 of its size, 2^20 away on every axis
        v, f = mc.sphere_interface(300)
        return 2.0 ** 20 + v * 2.0 ** -20, f
    return mc.sphere_interface(300)


@functools.lru_cache(maxsize=None)
def _scanner(name, n=4096):
    if name == "shifted":          # the sphere's rays moved with it (fp32 aims would collapse at 2^20)
        o, g = _scanner("sphere", n)
        return 2.0 ** 20 + o * 2.0 ** -20, 2.0 ** 20 + g * 2.0 ** -20
    return rc.scanner_rays(*_mesh(name), n)[:2]


@functools.lru_cache(maxsize=None)
def _grid_rays(name):
    """rays that exercise the walk: scanner rays, axis-parallel ones on and off cell boundaries, origins inside the box, lines that miss it"""
    v, f = _mesh(name)
    used = v[np.unique(f)]
    lo, hi = used.min(axis=0), used.max(axis=0)
    rng = np.random.default_rng(11)
    o, g = [x[:512] for x in _scanner(name)]
    parts = [(o, g)]
    for a in range(3):          # along each axis, both ways; a third of them start inside the box, some lie in the box's own planes
        p = lo + rng.random((96, 3)) * (hi - lo)
        p[:8] = lo + (hi - lo) * rng.integers(0, 8, (8, 3)) / 7.0
        q = p.copy()
        q[:, a] += np.where(rng.random(96) < 0.5, 1.0, -1.0) * (hi - lo)[a]
        p[:64, a] = np.where(rng.random(64) < 0.5, lo[a] - 0.3 * (hi - lo)[a], hi[a] + 0.3 * (hi - lo)[a])
        parts.append((p, q))
    inside = lo + rng.random((256, 3)) * (hi - lo)
    parts.append((inside, lo + rng.random((256, 3)) * (hi - lo)))
    off = hi + (hi - lo) * (0.5 + rng.random((64, 3)))          # beyond the box, running alongside it
    off2 = off.copy()
    off2[:, 0] = lo[0] - (hi - lo)[0]
    parts.append((off, off2))
    return np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts])


@functools.lru_cache(maxsize=None)
def _want(name, kind, t_min=0.0):
    o, g = _scanner(name) if kind == "scanner" else _grid_rays(name)
    return rc.first_hit(*_mesh(name), o, g, t_min)


@pytest.fixture
def current_device_calls(monkeypatch):
    """Records every call of torch.cuda.current_device() made from the package (the pattern of test_gpu_cell_labels.py)."""
    real = torch.cuda.current_device
    calls = []

    def spy():
        caller = inspect.stack()[1].filename
        if os.sep + "dgnn_amd" + os.sep in caller:
            calls.append(caller)
        return real()
    monkeypatch.setattr(torch.cuda, "current_device", spy)
    return calls


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _cast(mesh, o, g, **kw):
    from dgnn_amd import ops
    face, t, p, st = ops.ray_first_hit(mesh[0], mesh[1], o, g, return_stats=True, **kw)
    n = len(o)
    assert face.dtype == torch.int32 and t.dtype == p.dtype == torch.float64 and face.shape == t.shape == (n,) and p.shape == (n, 3)
    assert face.is_cuda and t.is_cuda and p.is_cuda and list(st) == list(rc.HIT_STATS)
    return face.cpu().numpy(), t.cpu().numpy(), p.cpu().numpy(), st


def _same(got, want):
    print("%d rays: %d faces differ, %d t differ; stats %s (model %s)" % (len(want[0]), (got[0] != want[0]).sum(), (_bits(got[1]) != _bits(want[1])).sum(),
                                                                        got[3], want[3]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])) and np.array_equal(_bits(got[2]), _bits(want[2]))
    assert got[3] == want[3]


# ---- plain rays --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "sphere", "tetrahedron"])
def test_scanner_rays_equal_the_model(name):
    want = _want(name, "scanner")
    assert want[3]["hits"] >= 0.99 * 4096
    _same(_cast(_mesh(name), *_scanner(name)), want)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_ray_counts(n):
    o, g = _scanner("cube", 4097)
    mesh = _mesh("cube")
    _same(_cast(mesh, o[:n], g[:n]), rc.first_hit(*mesh, o[:n], g[:n]))


def test_a_mesh_of_one_face():
    """and an unreferenced vertex that is NaN: it is not read"""
    mesh = _mesh("one_face")
    rng = np.random.default_rng(5)
    o = np.array([0.4, 0.4, 3.0]) + rng.random((300, 3)) * 0.2
    g = rng.random((300, 3))
    want = rc.first_hit(*mesh, o, g)
    assert 30 < want[3]["hits"] < 270
    for R in RESOLUTIONS:
        _same(_cast(mesh, o, g, grid_resolution=R), want)


@pytest.mark.parametrize("large_first", [True, False])
def test_one_face_over_every_cell_beside_faces_of_one_cell(large_first):
    """The entry lookup of the grid builder with very unequal boxes: one face spans the whole box [0, 1]^3, so it has R^3 entries, and
    20 small faces lie in one cell each, at 1, 2, 3 and 7 cells per axis; the large face is the first of the list or the last, which puts
    its run of entries at either end of the offsets the lookup searches."""
    import ctypes as C
    from dgnn_amd._lib import lib, ptr, stream_ptr
    rng = np.random.default_rng(23)
    slots = np.array([0.07, 0.21, 0.38, 0.62, 0.79, 0.93])          # +- 0.03 crosses no cell boundary k / 2, k / 3 or k / 7
    small = (slots[rng.integers(0, 6, (20, 1, 3))] + rng.uniform(-0.03, 0.03, (20, 3, 3))).reshape(60, 3)
    v = np.concatenate([np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]]), small])
    f = np.arange(63, dtype=np.int32).reshape(21, 3)
    if not large_first:
        f = np.roll(f, -1, axis=0)
    centroids = v[f].mean(axis=1)
    o = np.concatenate([np.repeat(centroids, 8, axis=0) + rng.choice([-2.0, 2.0], (168, 3)) * rng.uniform(0.8, 1.2, (168, 3)),
                        rng.uniform(-1.0, 2.0, (160, 3))])
    g = np.concatenate([np.repeat(centroids, 8, axis=0) + rng.uniform(-0.005, 0.005, (168, 3)), rng.uniform(0.0, 1.0, (160, 3))])
    want = rc.first_hit(v, f, o, g)
    assert {0, 20} <= set(want[0].tolist()) and want[3]["hits"] < len(o)          # the first and the last face are hit, and some rays miss
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    for R in (1, 2, 3, 7):
        scratch = torch.empty(int(lib().dgnn_ray_first_hit_scratch_bytes(21, R)), dtype=torch.uint8, device=vt.device)
        ne = C.c_int64(-1)
        assert lib().dgnn_ray_first_hit_plan(ptr(vt), 63, ptr(ft), 21, R, C.byref(ne), None, ptr(scratch), stream_ptr()) == 0
        assert ne.value == R ** 3 + 20
        _same(_cast((v, f), o, g, grid_resolution=R), want)


# ---- exact zeros -------------------------------------------------------------------------------------------------------------------
def _zero_rays(name):
    """aims at every vertex and every edge midpoint, from three origins each"""
    v, f = _mesh(name)
    tri = v[f]
    aims = np.concatenate([v[np.unique(f)]] + [0.5 * (tri[:, a] + tri[:, b]) for a, b in ((0, 1), (1, 2), (2, 0))])
    used = v[np.unique(f)]
    centre, ext = 0.5 * (used.min(axis=0) + used.max(axis=0)), used.max(axis=0) - used.min(axis=0)
    origins = centre + ext * np.array([[2.0, 1.25, -1.5], [-1.75, 0.5, 2.25], [0.25, -2.5, 0.125]])
    return np.repeat(origins, len(aims), axis=0), np.tile(aims, (3, 1))


@pytest.mark.parametrize("name", ["int_cube", "sphere"])
def test_aims_at_vertices_and_edge_midpoints(name):
    """integer cube: every zero is exact in fp64 too; sphere: the midpoints are rounded, the vertices exact"""
    mesh = _mesh(name)
    o, g = _zero_rays(name)
    want = rc.first_hit(*mesh, o, g)
    # (a rounded midpoint of a silhouette edge of the jagged sphere may fall off it: 34 of its 1515 rays miss)
    assert want[3]["exact_used"] > len(np.unique(mesh[1])) and want[3]["hits"] >= (len(o) if name == "int_cube" else 0.95 * len(o))
    for R in (1, 7, None):
        _same(_cast(mesh, o, g, grid_resolution=R), want)
    if name == "int_cube":          # every aim of the cube is hit at it, and exactly: t = 1 or nearer
        assert (want[1] <= 1).all() and (want[1] == 1).sum() > len(o) // 3


def test_rays_in_a_face_plane_and_along_an_edge():
    mesh = _mesh("int_cube")
    o = np.array([[-1.0, 1.0, 0.0], [-2.0, 0.0, 0.0], [-2.0, 4.0, 4.0], [1.0, 1.0, 0.0], [-3.0, -3.0, 0.0], [2.0, -1.0, 4.0], [0.0, -2.0, 1.0]])
    g = np.array([[0.0, 1.5, 0.0], [-1.0, 0.0, 0.0], [0.0, 4.0, 4.0], [3.0, 2.0, 0.0], [-1.0, -1.0, 0.0], [2.0, 0.0, 4.0], [0.0, -1.0, 1.0]])
    want = rc.first_hit(*mesh, o, g)
    v, f = mesh
    assert want[3]["hits"] == len(o) and want[1][1] == 2.0 and not (v[f[want[0][0]]][:, 2] == 0).all()
    for R in RESOLUTIONS:
        _same(_cast(mesh, o, g, grid_resolution=R), want)


# ---- front and back ----------------------------------------------------------------------------------------------------------------
def test_front_and_back():
    mesh = _mesh("int_cube")
    rng = np.random.default_rng(3)
    inside = 0.5 + 3.0 * rng.random((200, 3))
    aims = 4.0 * rng.random((200, 3))
    want = rc.first_hit(*mesh, inside, aims)
    assert want[3]["hits"] == 200                                          # from inside a closed mesh every ray hits
    _same(_cast(mesh, inside, aims), want)
    # origins exactly on the bottom face: its own crossing has t = 0 and is dropped, the far side is hit
    on = np.concatenate([np.array([[2.25, 1.5, 0.0], [2.0, 2.0, 0.0], [4.0, 4.0, 0.0], [0.0, 1.0, 0.0]]), np.c_[4.0 * rng.random((60, 2)), np.zeros(60)]])
    up = on + np.array([0.0, 0.0, 1.0])
    want = rc.first_hit(*mesh, on, up)
    assert (want[1] == 4.0).all() and (mesh[0][mesh[1][want[0]]][:, :, 2] == 4).all()
    _same(_cast(mesh, on, up), want)
    # pointing away: the line crosses the cube, the ray does not
    outside = np.array([5.0, 6.0, 7.0]) + rng.random((100, 3))
    away = 2 * outside - aims[:100]
    want = rc.first_hit(*mesh, outside, away)
    assert want[3] == dict(hits=0, skipped=0, degenerate=0, exact_used=0) and (want[0] == -1).all() and (want[1] == 0).all() and (want[2] == 0).all()
    _same(_cast(mesh, outside, away), want)
    # o == g is skipped, among live rays
    o, g = np.concatenate([outside[:5], inside[:5]]), np.concatenate([outside[:5], aims[:5]])
    want = rc.first_hit(*mesh, o, g)
    assert want[3]["skipped"] == 5 and want[3]["hits"] == 5
    _same(_cast(mesh, o, g), want)
    # t_min between the two hits of a ray that passes through
    o, g = outside, aims[:100] + 0.0
    near = rc.first_hit(*mesh, o, g)
    t_min = float(np.median(near[1]))
    far = rc.first_hit(*mesh, o, g, t_min)
    behind = near[1] <= t_min                                              # these rays lose their first hit and keep the way out
    assert near[3]["hits"] == 100 and behind.sum() == 50 and (far[1][behind & (far[0] >= 0)] > t_min).all() and (far[0][behind] != near[0][behind]).all()
    assert (far[0][behind] >= 0).sum() > 10 and np.array_equal(far[0][~behind], near[0][~behind])
    _same(_cast(mesh, o, g, t_min=t_min), far)
    exact = float(near[1][0])                                              # t == t_min is dropped
    _same(_cast(mesh, o[:1], g[:1], t_min=exact), rc.first_hit(*mesh, o[:1], g[:1], exact))
    assert rc.first_hit(*mesh, o[:1], g[:1], exact)[1][0] > exact


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "int_cube", "tetrahedron"])
def test_the_grid_does_not_matter(name):
    """axis-parallel rays, origins inside and outside the box, lines that miss it: every resolution gives the model's bits"""
    mesh = _mesh(name)
    o, g = _grid_rays(name)
    want = _want(name, "grid")
    assert 0.3 * len(o) < want[3]["hits"] <= len(o) - 64
    runs = [_cast(mesh, o, g, grid_resolution=R) for R in RESOLUTIONS]
    for got in runs:
        _same(got, want)


def test_a_small_face_in_a_later_cell_beats_a_large_one_met_first():
    """face 0 spans the whole box and lists itself in the first cell the ray visits, but is crossed at t = 23; face 1 sits in a later cell
    and is crossed at t = 6"""
    v = np.array([[24.0, 0.0, 0.0], [0.0, 24.0, 0.0], [0.0, 0.0, 24.0], [5.0, 0.5, 0.5], [5.0, 2.0, 0.5], [5.0, 0.5, 2.0]])
    f = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
    o, g = np.array([[-1.0, 1.0, 1.0], [-1.0, 3.0, 3.0]]), np.array([[0.0, 1.0, 1.0], [0.0, 3.0, 3.0]])
    want = rc.first_hit(v, f, o, g)
    assert list(want[0]) == [1, 0] and list(want[1]) == [6.0, 19.0]
    for R in (1, 2, 8, 24, 64, None):
        _same(_cast((v, f), o, g, grid_resolution=R), want)


# ---- the exact stage ---------------------------------------------------------------------------------------------------------------
def test_the_exact_stage_far_from_the_origin():
    """coordinates near 2^20 with features of 2^-20: the margin of the walk is 2^-24, a sixteenth of the mesh"""
    mesh = _mesh("shifted")
    o, g = _zero_rays("shifted")
    so, sg = [x[:1024] for x in _scanner("shifted")]
    o, g = np.concatenate([o, so]), np.concatenate([g, sg])
    want = rc.first_hit(*mesh, o, g)
    assert want[3]["exact_used"] > 100 and want[3]["hits"] > 0.9 * len(o)
    for R in (1, 7, 64, None):
        got = _cast(mesh, o, g, grid_resolution=R)
        assert got[3]["exact_used"] > 0
        _same(got, want)


# ---- degenerate faces ----------------------------------------------------------------------------------------------------------------
def test_degenerate_faces_and_a_degenerate_crossing():
    v, f = _mesh("int_cube")
    v2 = np.concatenate([v, [[2.0, 2.0, 2.0], [1.0, 1.0, 1.0], [3.0, 3.0, 3.0]]])
    f2 = np.concatenate([[[0, 0, 7], [0, 7, 7]], f, [[0, 3, 3], [8, 9, 10], [5, 5, 5]]]).astype(np.int32)
    o, g = _grid_rays("int_cube")
    o, g = np.concatenate([o, [[9.0, 9.0, 9.0]]]), np.concatenate([g, [[0.0, 0.0, 0.0]]])          # the last: along the line of face [8, 9, 10]
    want = rc.first_hit(v2, f2, o, g)
    plain = rc.first_hit(v, f, o, g)
    assert np.array_equal(want[0], np.where(plain[0] >= 0, plain[0] + 2, -1)) and np.array_equal(want[1], plain[1]) and want[3] == plain[3]
    for R in (1, 7, None):
        _same(_cast((v2, f2), o, g, grid_resolution=R), want)
    # a crossed face whose n . d cancels to 0 in fp64 (tests/test_ray_cast_model_cpu.py has the arithmetic), beside a face that is hit
    tv = np.array([[-0.25, -0.25, -0.75], [-0.25, 0.75, -0.75], [0.75, -0.25, 2.25], [-1.0, -1.0, 1.5], [1.0, -1.0, 1.5], [0.5, 2.0, 1.5]])
    tf = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
    o, g = np.zeros((3, 3)), np.array([[1.0 / 3.0, 0.0, 1.0], [0.0, 0.0, 1.0], [1.0 / 3.0, 0.0, 1.0]])
    o[2] = [-1.0 / 3.0, 0.0, -1.0]
    want = rc.first_hit(tv, tf, o, g)
    assert want[3]["degenerate"] == 2 and list(want[0]) == [1, 1, 1] and list(want[1]) == [1.5, 1.5, 1.25]          # rays 0 and 2 meet it, ray 1 has t = 0
    for R in (1, 2, 7, 64, None):          # the face spans many cells of the finer grids and is counted once
        _same(_cast((tv, tf), o, g, grid_resolution=R), want)


# ---- reruns, errors, device ----------------------------------------------------------------------------------------------------------
def test_reruns_are_bit_identical():
    mesh = _mesh("sphere")
    o, g = _grid_rays("sphere")
    runs = [_cast(mesh, o, g) for _ in range(2)]
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(runs[0][:3], runs[1][:3])) and runs[0][3] == runs[1][3]


def test_refusals_surface_as_errors():
    from dgnn_amd import ops
    from dgnn_amd._lib import DgnnError
    v, f = _mesh("cube")
    o, g = [x[:100] for x in _scanner("cube")]
    want = rc.first_hit(v, f, o, g)

    def good():
        _same(_cast((v, f), o, g), want)

    for bad_id in (-1, len(v)):
        bad = f.copy()
        bad[7, 1] = bad_id
        with pytest.raises(ValueError, match="out of range"):
            ops.ray_first_hit(v, bad, o, g)
        good()
    nan_v = v.copy()
    nan_v[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        ops.ray_first_hit(nan_v, f, o, g)
    unref = np.concatenate([v, [[np.nan, np.inf, 1e200]]])          # not referenced: not read
    _same(_cast((unref, f), o, g), want)
    for bad_value in (np.inf, -np.inf, np.nan):
        for which in (0, 1):
            rays = [o.copy(), g.copy()]
            rays[which][57, 2] = bad_value
            with pytest.raises(ValueError, match="non-finite"):
                ops.ray_first_hit(v, f, rays[0], rays[1])
    for big in (1e200, -1e200, 1e-200):
        huge = o.copy()
        huge[99, 0] = big
        with pytest.raises(DgnnError, match=r"2\^300"):
            ops.ray_first_hit(v, f, huge, g)
        huge_v = v.copy()
        huge_v[0, 0] = big
        with pytest.raises(DgnnError, match=r"2\^300"):
            ops.ray_first_hit(huge_v, f, o, g)
    good()
    with pytest.raises(ValueError, match="without faces"):
        ops.ray_first_hit(v, f[:0], o, g)
    with pytest.raises(ValueError, match="t_min"):
        ops.ray_first_hit(v, f, o, g, t_min=-1.0)
    for R in (0, -3, 1025):
        with pytest.raises(DgnnError, match="grid_resolution"):
            ops.ray_first_hit(v, f, o, g, grid_resolution=R)
    with pytest.raises(ValueError, match="origins"):
        ops.ray_first_hit(v, f, o[:5], g)
    good()


def test_rays_run_on_the_device_of_their_inputs(current_device_calls):
    from dgnn_amd import ops
    dev = torch.device("cuda", torch.cuda.device_count() - 1)          # a second device where there is one
    v, f = _mesh("cube")
    o, g = [x[:300] for x in _scanner("cube")]
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    face, t, p = ops.ray_first_hit(on(v), on(f), on(o), on(g))
    assert current_device_calls == []
    assert face.device == t.device == p.device == dev
    want = rc.first_hit(v, f, o, g)
    assert np.array_equal(face.cpu().numpy(), want[0]) and np.array_equal(_bits(t.cpu().numpy()), _bits(want[1]))
