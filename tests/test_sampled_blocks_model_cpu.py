"""The numpy model of the sampled block builder (tests/sampled_blocks_model.py): its structural properties, its agreement with the
oracle's full-neighbourhood restatement when nothing is dropped, and the uniformity of the key function.  No GPU."""
import itertools

import numpy as np
import pytest

import sampled_blocks_model as M

BATCHES = (1, 37, 128)
REG_SIZES = ([2] * 4, [3, 1, 2], [-1, 2, -1, 3])
IRR_SIZES = REG_SIZES + ([5] * 2,)


@pytest.fixture(scope="module")
def graphs():
    return {"regular": M.regular_graph(), "irregular": M.irregular_graph()}


def _batch(n, nb, seed):
    return np.random.default_rng(seed).permutation(n)[:nb].astype(np.int64)


def _cases():
    for name, sizes_list in (("regular", REG_SIZES), ("irregular", IRR_SIZES)):
        for sizes, nb in itertools.product(sizes_list, BATCHES):
            yield name, sizes, nb


def test_graphs_have_the_degrees_the_cases_need(graphs):
    ei, n = graphs["regular"]
    assert 1500 <= n <= 2600 and np.all(np.bincount(ei[1], minlength=n) == 4)
    assert np.array_equal(np.unique(np.stack([ei[1], ei[0]]), axis=1), np.unique(ei, axis=1))      # symmetric
    ei, n = graphs["irregular"]
    assert n == 600 and set(np.bincount(ei[1], minlength=n).tolist()) == set(range(13))


@pytest.mark.parametrize("name,sizes,nb", list(_cases()))
def test_model_properties(graphs, name, sizes, nb):
    ei, n = graphs[name]
    deg = np.bincount(ei[1], minlength=n)
    batch = _batch(n, nb, 11)
    n_id, adjs = M.sampled_blocks(ei, n, batch, sizes, seed=7, draw=3, with_off=True)
    assert len(adjs) == len(sizes) and np.array_equal(n_id[:nb], batch) and len(set(n_id.tolist())) == n_id.size
    n_src_outer = adjs[0][2][0]
    assert n_src_outer == n_id.size
    for hop, (e, e_id, (n_src, n_dst), off) in enumerate(adjs[::-1]):       # builder order: hop 0 = innermost
        size = sizes[hop]
        ids = n_id[:n_src]
        # every block edge is an edge of the graph with the right e_id
        assert np.array_equal(ei[0][e_id], ids[e[0]]) and np.array_equal(ei[1][e_id], ids[e[1]])
        assert len(set(e_id.tolist())) == e_id.size
        # grouped by target in target order, min(d, k) kept edges per target, in plan order (ascending edge position)
        assert np.array_equal(e[1], np.repeat(np.arange(n_dst), np.diff(off)))
        d = deg[ids[:n_dst]]
        assert np.array_equal(np.diff(off), d if size == -1 else np.minimum(d, size))
        for t in range(n_dst):
            seg = e_id[off[t]:off[t + 1]]
            assert np.all(np.diff(seg) > 0)
        # targets are a prefix of sources; new sources appear in first-appearance order
        assert n_src >= n_dst and (hop == 0 and n_dst == nb or hop > 0)
        new = e[0][e[0] >= n_dst]
        _, first = np.unique(new, return_index=True)
        assert np.array_equal(new[np.sort(first)], np.arange(n_dst, n_src))
    sizes_chain = [a[2] for a in adjs]
    for outer, inner in zip(sizes_chain[:-1], sizes_chain[1:]):
        assert outer[1] == inner[0]
    # a pure function of its arguments; another draw, another block (whenever something is dropped at all)
    again = M.sampled_blocks(ei, n, batch, sizes, seed=7, draw=3, with_off=True)
    assert np.array_equal(again[0], n_id) and all(np.array_equal(a[1], b[1]) for a, b in zip(again[1], adjs))
    if nb > 1:
        other = M.sampled_blocks(ei, n, batch, sizes, seed=7, draw=4, with_off=True)
        assert any(a[1].shape != b[1].shape or not np.array_equal(a[1], b[1]) for a, b in zip(other[1], adjs))
        seeded = M.sampled_blocks(ei, n, batch, sizes, seed=8, draw=3, with_off=True)
        assert any(a[1].shape != b[1].shape or not np.array_equal(a[1], b[1]) for a, b in zip(seeded[1], adjs))


def test_sizes_of_zero_or_below_minus_one_are_refused(graphs):
    ei, n = graphs["regular"]
    for bad in ([2, 0], [-2], [1, -3, 2]):
        with pytest.raises(ValueError):
            M.sampled_blocks(ei, n, np.arange(4), bad, 0, 0)


@pytest.mark.parametrize("name,sizes", [("regular", [4] * 4), ("regular", [4, -1, 7]), ("irregular", [12] * 3), ("irregular", [-1, 40])])
@pytest.mark.parametrize("nb", BATCHES)
def test_model_with_nothing_dropped_is_the_full_neighbour_sampler(graphs, name, sizes, nb):
    from oracle.pyg_semantics import neighbor_sampler_full
    ei, n = graphs[name]
    batch = _batch(n, nb, 5)
    n_id, adjs = M.sampled_blocks(ei, n, batch, sizes, seed=1, draw=9)
    ref_n_id, ref_adjs = neighbor_sampler_full(ei, n, batch, len(sizes))
    assert np.array_equal(n_id, ref_n_id) and len(adjs) == len(ref_adjs)
    for (e, e_id, size), (re, reid, rsize) in zip(adjs, ref_adjs):
        assert tuple(size) == tuple(rsize) and np.array_equal(e, re) and np.array_equal(e_id, reid)


def _chi2_bound(df):
    from scipy.stats import chi2
    return chi2.isf(1e-6, df)


def test_key_function_keeps_every_pair_of_four_equally_often(graphs):
    """k = 2 of d = 4: the 6 possible kept pairs over all targets x 8 draws against the uniform law (chi-square, 5 degrees of freedom)."""
    ei, n = graphs["regular"]
    pairs = {p: i for i, p in enumerate(itertools.combinations(range(4), 2))}
    counts = np.zeros(6, dtype=np.int64)
    for draw in range(8):
        for g in range(n):
            counts[pairs[tuple(M.kept(20240, draw, 0, g, 4, 2).tolist())]] += 1
    expected = counts.sum() / 6.0
    stat = ((counts - expected) ** 2 / expected).sum()
    print("pairs", counts.tolist(), "chi2", stat, "bound", _chi2_bound(5))
    assert counts.sum() == 8 * n and stat < _chi2_bound(5)


def test_key_function_keeps_every_in_edge_equally_often_per_degree_class(graphs):
    """k = 1 on the irregular graph: per in-degree d >= 2, the kept rank over all targets of that degree x 8 draws x 4 hops against the uniform
    law (chi-square, d - 1 degrees of freedom)."""
    ei, n = graphs["irregular"]
    deg = np.bincount(ei[1], minlength=n)
    for d in range(2, 13):
        counts = np.zeros(d, dtype=np.int64)
        for g in np.nonzero(deg == d)[0]:
            for draw in range(8):
                for hop in range(4):
                    counts[M.kept(99, draw, hop, int(g), d, 1)[0]] += 1
        expected = counts.sum() / float(d)
        stat = ((counts - expected) ** 2 / expected).sum()
        print("d", d, counts.tolist(), "chi2", stat, "bound", _chi2_bound(d - 1))
        assert expected >= 5 and stat < _chi2_bound(d - 1), (d, counts.tolist(), stat)
