"""The neighbour-joining definition as tests/nj_ref.py restates it, checked against itself on the CPU: the float64
statement makes the joins of exact rational arithmetic under the same tie rule, and it recovers integer tree metrics exactly."""
from fractions import Fraction

import numpy as np
import pytest

import nj_ref


def _int_matrix(n, hi, rng):
    U = np.triu(rng.integers(0, hi + 1, (n, n)), 1)
    return (U + U.T).astype(np.float64)


@pytest.mark.parametrize("hi", [1, 3, 10 ** 5])
@pytest.mark.parametrize("n", [4, 5, 7, 12, 24, 40])
def test_float_definition_makes_the_exact_joins(n, hi):
    """integer matrices, ties everywhere at the small ranges: same (a, b, D_ab) sequence; lengths within 1e-12 relative (only the
    division by 2 (r - 2) rounds)"""
    rng = np.random.default_rng(1000 * n + hi % 997)
    for _ in range(3 if n <= 24 else 1):
        D = _int_matrix(n, hi, rng)
        rec, last_ids, last_d = nj_ref.nj_records(D)
        joins, exact_edges = nj_ref.nj_exact(D.astype(np.int64).tolist())
        assert [(int(a), int(b), Fraction(float(d))) for a, b, d in zip(rec[0], rec[1], rec[2])] == joins
        parent, child, length = nj_ref.nj_edges(n, rec, last_ids, last_d)
        assert len(parent) == 2 * n - 3 == len(exact_edges)
        for p, c, x, (ep, ec, ex) in zip(parent.tolist(), child.tolist(), length.tolist(), exact_edges):
            assert (p, c) == (ep, ec)
            assert abs(Fraction(x) - ex) <= Fraction(1, 10 ** 12) * max(abs(ex), 1), (p, c, x, float(ex))


@pytest.mark.parametrize("n", [5, 64, 200])
def test_integer_tree_metrics_come_back_exactly(n):
    D, want = nj_ref.random_tree_metric(n, np.random.default_rng(n))
    parent, child, length = nj_ref.nj(D)
    assert nj_ref.splits_of(n, parent, child, length) == want          # every split, every length, as doubles


def test_small_cases_and_the_tie_rule():
    # n = 3: only the final step
    D = np.array([[0, 3, 5], [3, 0, 6], [5, 6, 0]], np.float64)
    parent, child, length = nj_ref.nj(D)
    assert parent.tolist() == [3, 3, 3] and child.tolist() == [0, 1, 2] and length.tolist() == [1.0, 2.0, 4.0]
    # n = 2, n = 1
    assert [x.tolist() for x in nj_ref.nj(np.array([[0, 7], [7, 0]], np.float64))] == [[0], [1], [7.0]]
    assert all(len(x) == 0 for x in nj_ref.nj(np.zeros((1, 1))))
    # all distances equal: every Q ties, the lowest ids join first and the new node (largest id) waits
    rec, last_ids, _ = nj_ref.nj_records(np.ones((6, 6)) - np.eye(6))
    assert list(zip(rec[0].tolist(), rec[1].tolist()))[0] == (0, 1)
    assert sorted(last_ids.tolist()) == last_ids.tolist()


def test_newick_parser_reads_quotes_and_nesting():
    nodes = nj_ref.parse_newick("(a:1,('b,''x':0.5,c:2e-05):3,d:-1);\n")
    assert nodes[0] == (None, None, None)
    assert [(p, lab, ln) for p, lab, ln in nodes[1:]] == [(0, "a", 1.0), (0, None, 3.0), (2, "b,'x", 0.5), (2, "c", 2e-05), (0, "d", -1.0)]
    sp = nj_ref.newick_splits(nodes, ["a", "b,'x", "c", "d"])
    assert sp[0b0110] == 3.0 and sp[0b0010] == 0.5 and sp[0b1110] == 1.0
