"""Scratch sizes of the training entry points (csrc/train.hip), pinned: every figure below was returned by the library BEFORE each backward
entry point's scratch layout was written once (one layout function read by the size query and by the entry point).  Host queries: no GPU."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def l():
    from dgnn_amd._lib import LIB_PATH, lib
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return lib()


# (n_src, n_dst, c_in, c_out, f_e) -> floats; the last two rows are invalid argument lists
STATIC_LAYER = [((1, 1, 29, 64, 20), 5508928), ((300, 257, 29, 64, 20), 5540160), ((5000, 3000, 64, 128, 20), 6289472),
                ((5000, 3000, 128, 128, 0), 2501700), ((-1, 1, 29, 64, 20), 16), ((300, 257, 0, 64, 20), 16)]
# (E, n_dst, c_in, c_out, k_e) -> floats; k_e == 0 and n_dst < 0 are invalid
UPDATED_LAYER = [((1, 1, 29, 64, 20), 8200), ((300, 257, 29, 64, 20), 15880), ((5000, 3000, 64, 128, 20), 417092),
                 ((5000, 3000, 128, 128, 0), 16), ((300, -1, 29, 64, 20), 16)]
# (n, c, hdim, n_out) -> floats; c == 0 and n < 0 are invalid
UPDATED_TAIL = [((257, 128, 64, 2), 42184), ((1, 64, 32, 2), 6408), ((257, 0, 64, 2), 64), ((-1, 128, 64, 2), 64)]


@pytest.mark.parametrize("args,want", STATIC_LAYER)
def test_static_layer_scratch_size(l, args, want):
    assert l.dgnn_sage_layer_train_scratch_elems(*args) == want


@pytest.mark.parametrize("args,want", UPDATED_LAYER)
def test_updated_layer_scratch_size(l, args, want):
    E, n_dst, c_in, c_out, k_e = args
    assert l.dgnn_sage_updated_train_scratch_elems(n_dst, E, c_in, c_out, k_e) == want


@pytest.mark.parametrize("args,want", UPDATED_TAIL)
def test_updated_tail_scratch_size(l, args, want):
    assert l.dgnn_updated_tail_scratch_elems(*args) == want


def test_static_model_scratch_size(l):
    """the default model on the blocks of tests/golden/static_f3_train_blocks.npz: four conv layers and the decoder's Linear + BatchNorm block
    (six widths), then with the decoder's output Linear riding in the call (seven); more than 8 layers is refused"""
    n_src, n_dst, widths = [1164, 686, 325, 116, 24, 24], [686, 325, 116, 24, 24, 24], [28, 64, 128, 128, 128, 64, 2]
    i64 = lambda v: (C.c_int64 * len(v))(*v)
    i32 = lambda v: (C.c_int32 * len(v))(*v)
    assert l.dgnn_static_train_scratch_elems(5, i64(n_src[:5]), i64(n_dst[:5]), i32(widths[:6]), 20) == 5786308
    assert l.dgnn_static_train_scratch_elems(6, i64(n_src), i64(n_dst), i32(widths), 20) == 5786564
    assert l.dgnn_static_train_scratch_elems(9, i64(n_src), i64(n_dst), i32(widths), 20) == 16
