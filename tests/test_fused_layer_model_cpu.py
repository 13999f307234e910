"""tests/fused_layer_model.py held to what it promises, without a GPU: the bounds that tests/test_gpu_fused_edges.py asserts are neither vacuous (a plain fp32
evaluation of the layer sits well inside them) nor blind (each planted defect of the kinds a fused kernel can have breaks them in the cell it was planted
in, and the report names that cell); ragged_graph holds the cells and groups it says it does; the restated tile geometry equals the sources' formulas and
the restated tile -> workgroup map gives the workgroup loads the edge sizes were chosen for.

The deep size 4 grid_cap TILE + TILE + 9 has 4 grid_cap + 2 tiles.  XCD 7 owns what is left of them behind seven shares of ceil(ntiles / 8) = grid_cap / 2 + 1
tiles: grid_cap / 2 - 5, five short of four tiles for each of its grid_cap / 8 workgroups.  So five workgroups of every launch (the last five slots of
XCD 7) own 3 tiles and every other one owns 4 or 5; test_workgroup_loads_at_the_edge_sizes asserts exactly that."""
import numpy as np
import pytest
import torch

import fused_layer_model as fm

SHAPES = [(28, 64), (20, 128), (48, 128), (64, 64), (96, 128), (128, 128)]
DEEP = 32809                       # the smallest deep size (TILE 32, grid cap 256)
SIZES = [1, 33, 300, DEEP]


def layer_f32(x, ea, ei, n_dst, We, be, Wj, bj, Wi, scale, shift, relu=True, defect=None, cell=None):
    """the layer in plain torch float32 (every product and sum rounded to fp32, in torch's order), with one planted defect in `cell`"""
    src, dst = ei[0], ei[1]
    phi = ea @ We.t() + be
    m = x[src] * phi
    deg = torch.bincount(dst, minlength=n_dst)
    if defect == "shifted_eid":                     # the cell's edge-attribute rows come from the next edge each
        e = torch.nonzero(dst == cell).flatten()
        m[e] = x[src[e]] * (ea[(e + 1) % ea.size(0)] @ We.t() + be)
    a = torch.zeros(n_dst, x.size(1)).index_add_(0, dst, m) / deg.clamp(min=1).unsqueeze(1).float()
    own = x[:n_dst].clone()
    if defect == "degree_3_over_4":
        assert int(deg[cell]) == 3
        a[cell] = a[cell] * 3 / 4
    if defect == "empty_cell_gets_a_mean":          # an in-degree-0 cell is handed its neighbour's mean
        assert int(deg[cell]) == 0
        a[cell] = a[cell + 1] if cell + 1 < n_dst else a[cell - 1]
    if defect == "fp16_no_low_part":                # the row's operands with 11 significand bits and nothing to compensate
        h = lambda v: v.half().float() if float(v.abs().max()) < 6e4 else (v / 1024).half().float() * 1024
        a[cell], own[cell] = h(a[cell]), h(own[cell])
    y = a @ Wj.t() + own @ Wi.t()
    if bj is not None:
        y = y + bj
    if scale is not None:
        y = y * scale + shift
    return torch.relu(y) if relu else y


def _case(c_in, c_out, n, seed=0):
    n_src = n + 37
    ei = torch.from_numpy(fm.ragged_graph(n, n_src, 1000 * c_in + n + seed))
    inp = fm.layer_inputs(c_in, c_out, n_src, ei.size(1), n + c_in + c_out)
    return ei, inp


_CASES = {}


def _cached(c_in, c_out, n):
    key = (c_in, c_out, n)
    if key not in _CASES:
        ei, inp = _case(c_in, c_out, n)
        x, ea = inp[0], inp[1]
        ref, mag = fm.reference(x, ea, ei, n, *inp[2:], relu=True)
        _CASES[key] = (ei, inp, ref, mag)
    return _CASES[key]


@pytest.mark.parametrize("c_in,c_out", SHAPES)
@pytest.mark.parametrize("n", SIZES)
def test_plain_fp32_stays_inside_every_bound(c_in, c_out, n):
    ei, inp, ref, mag = _cached(c_in, c_out, n)
    x, ea = inp[0], inp[1]
    out = layer_f32(x, ea, ei, n, *inp[2:])
    deg = fm.in_degrees(ei, n)
    worst, rep = fm.check_elements(out, ref, fm.K_F32 * mag + 1e-30, deg, 4)
    print("fp32 evaluation %d -> %d, n = %d: err / (2^-20 mag) <= %.3f" % (c_in, c_out, n, worst))
    assert rep is None and worst <= 0.5, (worst, rep)        # inside the tighter of the two bounds with room to spare, so inside 2^-19 too
    # the epilogue switches of the reference
    for kw in (dict(bj=None), dict(scale=None, shift=None), dict(relu=False), dict(bj=None, scale=None, shift=None, relu=False)):
        We, be, Wj, bj, Wi, scale, shift = inp[2:]
        args = dict(bj=bj, scale=scale, shift=shift, relu=True)
        args.update(kw)
        if n > 300:
            break
        r2, m2 = fm.reference(x, ea, ei, n, We, be, Wj, args["bj"], Wi, args["scale"], args["shift"], relu=args["relu"])
        o2 = layer_f32(x, ea, ei, n, We, be, Wj, args["bj"], Wi, args["scale"], args["shift"], relu=args["relu"])
        w2, rep2 = fm.check_elements(o2, r2, fm.K_F32 * m2 + 1e-30)
        assert rep2 is None, (kw, w2, rep2)


def _cell_with(deg, value, lo=0):
    c = np.nonzero(deg == value)[0]
    c = c[c >= lo]
    assert c.size, "no cell of in-degree %d" % value
    return int(c[0])


@pytest.mark.parametrize("c_in,c_out", SHAPES)
@pytest.mark.parametrize("defect,degree", [("degree_3_over_4", 3), ("shifted_eid", 5), ("fp16_no_low_part", 40), ("empty_cell_gets_a_mean", 0)])
def test_planted_defects_break_the_bound_in_their_cell(c_in, c_out, defect, degree):
    n = 300
    ei, inp, ref, mag = _cached(c_in, c_out, n)
    x, ea = inp[0], inp[1]
    deg = fm.in_degrees(ei, n)
    cell = _cell_with(deg, degree, lo=64)
    out = layer_f32(x, ea, ei, n, *inp[2:], defect=defect, cell=cell)
    for kappa in (fm.K_F32, fm.K_F16):
        worst, rep = fm.check_elements(out, ref, kappa * mag + 1e-30, deg, 16)
        assert rep is not None and worst > 1.0, (defect, kappa)
        assert rep["cell"] == cell and rep["in_degree"] == degree and rep["cells_outside"] == 1 and rep["group_regular"] is False, rep
        assert rep["outside"] >= 1 and 0 <= rep["column"] < c_out


@pytest.mark.parametrize("c_in", [96, 128])
@pytest.mark.parametrize("defect,degree", [("degree_3_over_4", 3), ("shifted_eid", 5), ("empty_cell_gets_a_mean", 0)])
def test_planted_defects_break_the_logit_bound_in_their_cell(c_in, defect, degree):
    """behind the decoder the bound is the worst case of 128 x 64 sums whose errors in fact average out (a plain fp32 evaluation measures a few 1e-4 of it): it
    holds a cell's logits to the right neighbours, attribute rows and divisor, not to the last bits of the arithmetic -- the layer's own rows are held to those"""
    n = 300
    ei, inp, ref, mag = _cached(c_in, 128, n)
    dec = fm.decoder_inputs(n + c_in)
    lref, lmag = fm.decoder_reference(ref, mag, *dec)
    deg = fm.in_degrees(ei, n)
    cell = _cell_with(deg, degree, lo=64)
    W0, b0, s1, h1, W3, b3 = dec
    logits = lambda y: torch.relu((y @ W0.t() + b0) * s1 + h1) @ W3.t() + b3
    worst, rep = fm.check_elements(logits(layer_f32(inp[0], inp[1], ei, n, *inp[2:])), lref, fm.K_LOGIT * lmag + 1e-30, deg, 4)
    assert rep is None and worst <= 0.01, (worst, rep)
    worst, rep = fm.check_elements(logits(layer_f32(inp[0], inp[1], ei, n, *inp[2:], defect=defect, cell=cell)), lref, fm.K_LOGIT * lmag + 1e-30, deg, 4)
    assert rep is not None and rep["cell"] == cell and rep["cells_outside"] == 1 and rep["in_degree"] == degree, (worst, rep)


def test_the_report_counts_a_nan_as_outside():
    ref, mag = torch.ones(3, 4, dtype=torch.float64), torch.ones(3, 4, dtype=torch.float64)
    out = ref.clone().float()
    assert fm.check_elements(out, ref, fm.K_F32 * mag) == (0.0, None)
    out[2, 1] = float("nan")
    worst, rep = fm.check_elements(out, ref, fm.K_F32 * mag, np.array([4, 4, 7]), 2)
    assert worst == float("inf") and rep["cell"] == 2 and rep["column"] == 1 and rep["in_degree"] == 7 and rep["outside"] == 1


@pytest.mark.parametrize("n", [1, 3, 300, 9 * 64 + 9, DEEP])
def test_ragged_graph_has_what_it_promises(n):
    n_src = n + 37
    ei = fm.ragged_graph(n, n_src, 5 + n)
    deg = fm.in_degrees(ei, n)
    assert ei.dtype == np.int64 and ei.shape[0] == 2 and ei[1].max() < n and 0 <= ei[0].min() and ei[0].max() < n_src
    assert np.array_equal(deg, fm.ragged_degrees(n, 5 + n))
    if n == 1:
        assert deg[0] == 40                               # the one-cell graph is a long per-lane loop
    if n == 3:
        assert deg[2] == 0
    if n >= 300:
        assert (ei[0] >= n).any()                         # source rows that are no destinations
        # edge columns are shuffled: the stable sort by destination that the plan does is no identity
        eid = np.argsort(ei[1], kind="stable")
        assert not np.array_equal(eid, np.arange(eid.shape[0]))
        assert (ei[0] == ei[1]).any()                     # self-loops
        key = ei[0] * n + ei[1]
        assert np.unique(key).shape[0] < key.shape[0]     # duplicate edges
        for tpw in (4, 8, 16):
            reg = fm.group_regular(deg, tpw)
            assert reg.any() and (~reg).any()
        # both kinds of 16-cell group, and per ragged stretch the cells 0 / 40 / 3 / 5, the latter two closing an otherwise regular group of 16
        g16 = deg[: n // 16 * 16].reshape(-1, 16)
        assert (g16 == 4).all(1).any() and (g16 != 4).any(1).any()
        for s in range(n // 64):
            d = deg[64 * s: 64 * s + 64]
            if not fm.stretch_is_ragged(s):
                assert (d == 4).all()
                continue
            assert d[fm.OFF_40] == 40 and d[fm.OFF_0] == 0 and d[fm.OFF_3] == 3 and d[fm.OFF_5] == 5
            assert (d[32:47] == 4).all() and (d[48:63] == 4).all() and d[:32].max() == 40 and ((d[:32] >= 0) & ((d[:32] <= 9) | (d[:32] == 40))).all()
    reg = fm.regular_graph(n, n_src, 3)
    assert np.array_equal(reg[1], np.repeat(np.arange(n), 4)) and reg[0].max() < n_src


def test_stretches_alternate_in_the_thue_morse_order():
    kinds = fm.stretch_is_ragged(np.arange(16))
    assert kinds.tolist() == [True, False, False, True, False, True, True, False, False, True, True, False, True, False, False, True]
    assert bool(fm.stretch_is_ragged(0)) is True


def test_geometry_table_is_the_sources_formulas():
    for (cp, c_out, family), row in fm.TWO_PHASE.items():
        assert fm.geometry(cp, c_out, family) == row, (cp, c_out, family)
    # every shape the GPU suite runs maps onto a row
    for c_in, c_out in [(28, 64), (20, 128), (32, 128), (64, 64), (48, 128), (96, 128), (29, 64), (100, 128), (64, 128), (128, 128), (72, 128)]:
        for mode in fm.MODES:
            fam = fm.family_of(c_in, c_out, mode, ws_enabled=False)
            assert (fm.cin_pad(c_in), c_out, fam) in fm.TWO_PHASE
    assert fm.family_of(29, 64, "f16x2") == "fused" and fm.family_of(100, 128, "bf16x3f") == "fused" and fm.family_of(48, 128, "f16x2") == "mfma"
    assert fm.family_of(128, 128, "f16x2") == "ws" and fm.family_of(128, 128, "f16x2", ws_enabled=False) == "mfma" and fm.family_of(96, 128, "f16x2") == "mfma"
    assert fm.family_of(48, 128, "f16x2", rows_16_byte=False) == "fused" and fm.family_of(28, 64, "f16x2d", rows_16_byte=False) == "mfma"


def _hand_overs(n, tile, tpw, cap, deg):
    """(some wave goes matrix-core -> per-lane between two consecutive tiles of its workgroup, some wave goes the other way)"""
    reg = fm.group_regular(deg, tpw)
    to_lane = to_mfma = False
    for tiles in fm.tiles_of_workgroups(n, tile, cap):
        for t0, t1 in zip(tiles[:-1], tiles[1:]):
            for w in range(tile // tpw):
                i0, i1 = t0 * tile + w * tpw, t1 * tile + w * tpw
                if i1 >= n:
                    continue
                to_lane |= bool(reg[i0] and not reg[i1])
                to_mfma |= bool(reg[i1] and not reg[i0])
    return to_lane, to_mfma


@pytest.mark.parametrize("key", sorted(fm.TWO_PHASE))
def test_workgroup_loads_at_the_edge_sizes(key):
    tile, tpw, cap = fm.TWO_PHASE[key]
    sizes = fm.edge_sizes(tile, tpw, cap)
    assert sizes == [1, tpw - 1, tpw + 1, tile + 1, 9 * tile + 9, 4 * cap * tile + tile + 9] and 32809 <= sizes[-1] <= 131145
    for n in sizes:                                      # the map hands out every tile once
        wgs = fm.tiles_of_workgroups(n, tile, cap)
        assert sorted(t for w in wgs for t in w) == list(range(-(-n // tile))) and len(wgs) <= cap
    loads = sorted(set(len(w) for w in fm.tiles_of_workgroups(sizes[4], tile, cap)))
    assert loads == [0, 1, 2], loads                     # ten tiles: workgroups with 0, 1 and 2 tiles in one launch
    deep = [len(w) for w in fm.tiles_of_workgroups(sizes[5], tile, cap)]
    assert len(deep) == cap and sizes[5] % tile == 9
    short = [b for b, k in enumerate(deep) if k < 4]
    assert min(deep) == 3 and max(deep) == 5 and len(short) == 5 and all(b & 7 == 7 and b >> 3 >= cap // 8 - 5 for b in short), (min(deep), max(deep), short)
    # the ragged graph hands every gather group size both ways between the two paths, at ten tiles or at the deep size
    both = [False, False]
    for n in sizes[4:]:
        a, b = _hand_overs(n, tile, tpw, cap, fm.ragged_degrees(n, 11))
        both = [both[0] or a, both[1] or b]
    assert both == [True, True], both
    a, b = _hand_overs(sizes[5], tile, tpw, cap, fm.ragged_degrees(sizes[5], 11))
    assert a and b
