"""tests/fitch_ref.py, the restated definition of DESIGN.md 3.20, against exhaustive search over the internal states, and the
properties the definition promises."""
import numpy as np
import pytest

import fitch_ref as fr

A, C_, G, T, N = 1, 2, 4, 8, 15


def _d(masks, i, j):
    return int(((masks[i] & masks[j]) == 0).sum())


@pytest.mark.parametrize("n", [3, 4, 5, 6, 7])
def test_count_equals_the_exhaustive_minimum(n):
    rng = np.random.default_rng(100 + n)
    trees = 40 if n < 7 else 12
    for _ in range(trees):
        parent, child = fr.random_tree(n, rng)
        masks = rng.integers(1, 16, (n, 6))
        got = fr.fitch(parent, child, masks)
        assert np.array_equal(got["site_changes"], got["site_cost"])
        for s in range(masks.shape[1]):
            assert got["site_changes"][s] == fr.exhaustive_minimum(parent, child, masks[:, s]), (parent, child, masks[:, s])
        assert (got["site_changes"] >= got["site_minimum"]).all()
        assert got["edge_changes"].sum() == got["site_changes"].sum() == got["total"] == len(got["entries"])


def test_states_lie_in_the_masks_and_n_never_changes():
    rng = np.random.default_rng(5)
    n = 9
    parent, child = fr.random_tree(n, rng)
    masks = rng.integers(1, 16, (n, 40))
    masks[3] = N
    got = fr.fitch(parent, child, masks)
    for s, e, info in got["entries"]:
        fp, fc = info & 15, info >> 4
        assert fp != fc and bin(fp).count("1") == 1 and bin(fc).count("1") == 1
        c = int(child[e])
        if c < n:
            assert fc & masks[c, s] and c != 3
    # entries: sites ascending, walk order within a site
    rank = {e: k for k, e in enumerate(fr.walk_order(n, len(parent)))}
    keys = [(s, rank[e]) for s, e, _ in got["entries"]]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_small_n():
    e = np.zeros(0, np.uint32)
    got = fr.fitch(e, e, np.array([[A, N, 3]]))
    assert got["total"] == 0 and got["entries"] == [] and list(got["site_minimum"]) == [0, 0, 0]
    masks = np.array([[A, A, 3, N, 6, C_], [A, C_, 6, G, 9, N]])
    got = fr.fitch([0], [1], masks)
    assert list(got["site_changes"]) == [0, 1, 0, 0, 1, 0] and got["total"] == _d(masks, 0, 1) == 2
    assert got["entries"] == [(1, 0, A | (C_ << 4)), (4, 0, C_ | (A << 4))]
    assert list(got["site_minimum"]) == [0, 1, 0, 0, 1, 0]
    masks = np.array([[A, A, A], [A, C_, C_], [A, C_, G]])
    got = fr.fitch([3, 3, 3], [0, 1, 2], masks)
    assert list(got["site_changes"]) == [0, 1, 2] and list(got["edge_changes"]) == [1, 1, 1]
    # site 1: S_xy = {A, C}, S_T = {C}: the change is on the edge to sample 0; site 2: S_T = S_xy = {A, C}, f_T = A
    assert got["entries"] == [(1, 0, C_ | (A << 4)), (2, 1, A | (C_ << 4)), (2, 2, A | (G << 4))]


def test_all_n_common_base_and_the_overlapping_pairs():
    rng = np.random.default_rng(11)
    n = 6
    parent, child = fr.random_tree(n, rng)
    masks = rng.integers(1, 16, (n, 4))
    masks[:, 0] = N                                   # all N
    masks[:, 1] |= G                                  # G is in every mask
    got = fr.fitch(parent, child, masks)
    assert got["site_changes"][0] == 0 and got["site_changes"][1] == 0
    assert got["site_minimum"][0] == 0 and got["site_minimum"][1] == 0
    # {A,C}, {C,G}, {A,G}: pairwise overlapping, no pair "differs", and still one change -- and a minimum of 1
    masks = np.array([[A | C_], [C_ | G], [A | G]])
    assert all(_d(masks, i, j) == 0 for i in range(3) for j in range(3))
    got = fr.fitch([3, 3, 3], [0, 1, 2], masks)
    assert got["total"] == 1 and list(got["site_minimum"]) == [1]
    assert fr.exhaustive_minimum([3, 3, 3], [0, 1, 2], masks[:, 0]) == 1


def test_minimum_by_enumeration():
    cols = np.array([[A, A, A, A, 3], [A, C_, C_, C_, 12], [A, C_, G, G, N], [A, 3, 5, T, N]])
    assert list(fr.minimum(cols)) == [0, 1, 2, 3, 1]


@pytest.mark.parametrize("n", [2, 3, 5, 8, 12])
def test_path_changes_are_at_least_the_snp_distance(n):
    rng = np.random.default_rng(n)
    parent, child = fr.random_tree(n, rng)
    masks = rng.choice([A, C_, G, T, A | G, C_ | T, N], (n, 30), p=[.3, .2, .2, .15, .05, .05, .05])
    got = fr.fitch(parent, child, masks)
    for i in range(n):
        for j in range(i + 1, n):
            path = sum(fr.path_changes(parent, child, got["entries"], n, i, j, s) for s in range(masks.shape[1]))
            assert path >= _d(masks, i, j), (i, j)
    if n == 2:
        assert got["total"] == _d(masks, 0, 1)


def test_tree_builders_give_the_shape():
    for n in (3, 4, 5, 9, 64):
        for p, c in (fr.caterpillar(n), fr.balanced(n), fr.random_tree(n, np.random.default_rng(n))):
            assert len(p) == 2 * n - 3 and sorted(c) == list(range(2 * n - 3))
            for t in range(n - 3):
                assert p[2 * t] == p[2 * t + 1] == n + t and c[2 * t] < c[2 * t + 1] < n + t
            assert list(p[-3:]) == [2 * n - 3] * 3 and c[-3] < c[-2] < c[-1]
