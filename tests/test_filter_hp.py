"""tests/golden/filter_hp_golden.json -- the recombination filter's smallest surviving spans and the filtered distances of crafted
pairs from the definition at 50 digits (tests/hp_filter.py) -- against a fresh evaluation of a sample of it, and the oracle
(oracle/tracs_oracle.c: the filter in double, its binomial CDF from a continued fraction) against all of it.

Mutation check (run once by hand against the oracle, not part of the suite): with orc_binomial_cdf's result lowered by the
last term of the upper-tail sum, C(n, n) p^n -- or with 1 added to one reachable cell of a fixture row --
test_oracle_equals_the_fixture_on_every_case and test_oracle_tail_decides_as_the_definition fail."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "golden", "filter_hp_golden.json")
EDGES = ((9000, 90), (9000, 91), (120000, 1200), (120000, 1201), (600000, 60), (600000, 61), (1000000, 65536), (1000000, 65537))


@pytest.fixture(scope="module")
def fx():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def H():
    pytest.importorskip("mpmath")
    import hp_filter
    return hp_filter


@pytest.fixture(scope="module")
def sites(fx, H):
    """the crafted sites of every case, built once"""
    return {(c["L"], c["d"]): H.boundary_positions(c["L"], c["d"], c["row"]) for c in fx["cases"]}


def test_fixture_header_and_coverage(fx):
    cases = fx["cases"]
    assert fx["margin"] == 1e-9 and fx["digits"] >= 40
    m = fx["measured"]
    assert m["ill_cells"] == 0
    assert m["min_relative_margin"] == min(c["min_margin"] for c in cases) > 1e3 * fx["margin"]
    assert 0 < m["oracle_max_error_over_threshold"] <= fx["margin"]
    assert m["covered_per_case"] == {"%d/%d" % (c["L"], c["d"]): c["covered"] for c in cases}
    want = {9000: [2, 3, 90, 91, 600, 1500], 120000: [2, 7, 12, 37, 40, 300, 1200, 1201, 9000], 600000: [45, 60, 61, 118],
            1000000: [196, 4200, 65536, 65537, 70000, 150000]}
    assert {L: [c["d"] for c in cases if c["L"] == L] for L in want} == want and len(cases) == sum(map(len, want.values()))
    for c in cases:
        assert len(c["row"]) == 62 and c["expected"] <= c["d"]
        # boundary k covered: every attainable one up to 2 (d >= 20) and 8 (d >= 600) -- a sparse pair has fewer than 8
        # reachable k whatever its sites (120 000 / 1 200: k = 2 .. 6 only)
        assert c["covered"] >= min(8 if c["d"] >= 600 else 2 if c["d"] >= 20 else 0, c["attainable"]), c
        assert c["attainable"] >= 2 or c["d"] < 20
    assert sum(c["covered"] >= 8 for c in cases if c["d"] >= 600) >= 7
    # the half window on either side of its edges: the clamps at 50 and 5 000, and L / (2 d) a whole number
    wh = {(c["L"], c["d"]): c["wh"] for c in cases}
    assert (wh[9000, 90], wh[9000, 91], wh[120000, 1200], wh[120000, 1201]) == (51, 50, 51, 50)
    assert (wh[120000, 12], wh[120000, 40], wh[600000, 60], wh[600000, 61]) == (5000, 1501, 5000, 4919)


def test_builder_and_definition_reproduce_the_fixture(fx, H, sites):
    cases = {(c["L"], c["d"]): c for c in fx["cases"]}
    rest = sorted(set(cases) - set(EDGES))
    rng = np.random.default_rng(5)
    todo = list(EDGES) + [rest[int(i)] for i in rng.choice(len(rest), 5, replace=False)]
    for L, d in todo:
        c = cases[L, d]
        _, _, wh = H.window(L, d)
        row = H.row(L, d)
        assert wh == c["wh"] and row == c["row"], (L, d)
        pos = sites[L, d]
        assert len(pos) == d and len(set(pos)) == d and pos == sorted(pos) and 0 <= pos[0] and pos[-1] < L
        kept, cells, ill, margin = H.filter_positions(pos, L)
        assert ill == 0 and kept == c["expected"] and len(cells) == c["cells"], (L, d, kept, ill)
        assert margin >= c["min_margin"] >= fx["measured"]["min_relative_margin"]
        hit = H.must_hit(L, d, row)
        assert len(hit) == 2 * c["covered"] and all(x in cells for x in hit), (L, d)
        for k, n in hit[0::2]:
            assert cells[k, n] and not cells[k, n - 1]           # kept at n*, dropped one site shorter
        if d > 3:
            assert pos[0] == 0 and pos[-1] == L - 1               # the clamps of the window at both ends
        assert H.choose_probe(L, d) == tuple(c["probe"])


def test_oracle_equals_the_fixture_on_every_case(fx, oracle, sites):
    for c in fx["cases"]:
        assert oracle.filter_recomb_positions(sites[c["L"], c["d"]], c["L"]) == c["expected"], (c["L"], c["d"])


def test_oracle_tail_decides_as_the_definition(fx, H, oracle):
    """|(1 - cdf) - tail| <= MARGIN thr at n* and n* - 1 of every row: with no cell inside the margin, the oracle's double decision is
    the definition's.  The largest ratio seen is what the fixture's header and DESIGN.md section 4 quote."""
    worst, n_cells = 0.0, 0
    with H.mp.workdps(H.DPS):
        for c in fx["cases"]:
            L, d = c["L"], c["d"]
            p, thr, _ = H.window(L, d)
            for k, ns in enumerate(c["row"], start=2):
                for n in ((ns, ns - 1) if ns is not None else ()):
                    err = float(abs(H.mpf(1.0 - oracle.binomial_cdf(n, p, k)) - H.tail(n, k, p)) / H.mpf(thr))
                    assert err <= H.MARGIN, (L, d, k, n, err)
                    assert (1.0 - oracle.binomial_cdf(n, p, k) >= thr) == (n == ns), (L, d, k, n)
                    worst, n_cells = max(worst, err), n_cells + 1
    print("oracle vs the definition: %d boundary cells, largest |error| / thr %.3g" % (n_cells, worst))
    assert n_cells > 400 and worst <= 2 * fx["measured"]["oracle_max_error_over_threshold"]


def test_oracle_half_window_in_double(fx, H, oracle):
    """wh = clamp(int(1.0 / p / 2.0 + 1), 50, 5000) as the oracle computes it, on every (L, d): two SNPs wh apart share a window,
    two wh + 1 apart do not, and the fixture's probe gives a different filtered distance for the two."""
    for c in fx["cases"]:
        L, d = c["L"], c["d"]
        _, _, wh = H.window(L, d)
        shape, at_wh, beyond = c["probe"]
        assert wh == c["wh"] and at_wh != beyond
        assert oracle.filter_recomb_positions(H.probe_positions(L, d, shape, wh), L) == at_wh, (L, d)
        assert oracle.filter_recomb_positions(H.probe_positions(L, d, shape, wh + 1), L) == beyond, (L, d)
