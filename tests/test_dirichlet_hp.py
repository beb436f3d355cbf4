"""tests/golden/dirichlet_hp_golden.json -- find_dirichlet_priors' alphas and iteration counts, and digamma on a grid, from their
definitions at 50 digits (tests/hp_dirichlet.py) -- against a fresh evaluation of a sample of it, and the oracle's scipy restatement
(oracle.find_dirichlet_priors) against all of it: the same iteration count on every case, and alphas within twice the error recorded
when the fixture was written.

Mutation check (run once by hand against the oracle, not part of the suite): with the clamp applied on the converged path too
(6 cases fail, two_converged among them), with one iteration more after the stopping rule holds (every converging case fails) or with
LOO's max |delta| turned into the sum (d25_LOO_1e-05 fails) test_oracle_against_the_fixture_on_every_case fails."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "golden", "dirichlet_hp_golden.json")
CHEAPEST = ("cut6", "d25_max_iter_33")


@pytest.fixture(scope="module")
def fx():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def H():
    import hp_dirichlet                 # imports mpmath only inside the functions that evaluate at 50 digits
    return hp_dirichlet


def _case(fx, name):
    return next(c for c in fx["cases"] if c["name"] == name)


def test_fixture_header_and_coverage(fx, H):
    cases = {c["name"]: c for c in fx["cases"]}
    assert fx["digits"] >= 50 and fx["ill"] == 1e-6 == H.ILL
    for c in cases.values():
        assert c["margin"] is None or c["margin"] >= fx["ill"], c["name"]          # no ill case
        assert (c["margin"] is None) == (c["iters"] == 0)
        assert len(c["alphas"]) == c["K"] == len(fx["tables"][c["table"]][0]) - 1
        hi = [a[0] for a in c["alphas"]]
        assert c["iters"] <= c["max_iter"] and (hi == sorted(hi, reverse=True) or c["kept_rows"] <= 5)
    # what the cases reach
    for tab in ("d8", "d25", "d200"):
        for method in ("FPI", "LOO"):
            for tol in ("1e-05", "1e-11"):
                assert cases["%s_%s_%s" % (tab, method, tol)]["K"] == 4
    assert [cases["k%d" % K]["K"] for K in (2, 3, 5, 8)] == [2, 3, 5, 8]
    assert max(max(r[:-1]) for r in fx["tables"]["c60k"]) > 60000 and max(max(r[:-1]) for r in fx["tables"]["c3e8"]) > 3e8
    assert max(max(r[:-1]) for r in fx["tables"]["c3e8"]) < 2 ** 30
    assert [cases["d25_max_iter_%d" % m]["iters"] for m in (0, 1, 31, 32, 33, 64, 65)] == [0, 1, 31, 32, 33, 64, 65]
    assert cases["d25_FPI_1e-05"]["iters"] < 1000 and cases["d25_FPI_1e-11"]["iters"] == 1000     # a convergence and a max_iter stop
    # two alleles only: the two lowest alphas are exactly 0 after a convergence and exactly the clamp after max_iter
    conv, capped = cases["two_converged"], cases["two_max_iter"]
    assert conv["iters"] < conv["max_iter"] and conv["alphas"][2:] == [[0.0, 0.0], [0.0, 0.0]]
    assert capped["iters"] == capped["max_iter"] and capped["alphas"][2:] == [[1e-16, 0.0], [1e-16, 0.0]]
    # the 5 / 6 kept-rows boundary
    assert cases["cut5"]["kept_rows"] == 5 and cases["cut5"]["alphas"] == [[0.0, 0.0]] * 3 + [[1.0, 0.0]] and cases["cut5"]["iters"] == 0
    assert cases["cut6"]["kept_rows"] == 6 and cases["cut6"]["iters"] > 0 and cases["cut6"]["alphas"][0][0] > 1.0
    # the filter at equality: 400 rows (19, 1, 0, 0) are kept, 400 rows (39, 1, 0, 0) and 400 rows without counts are dropped
    base, keep19, drop39, zero = (cases[n + "_filter_0.05"] for n in ("base", "keep19", "drop39", "zero"))
    assert keep19["kept_rows"] == base["kept_rows"] + 400 and drop39["kept_rows"] == zero["kept_rows"] == base["kept_rows"]
    assert drop39["alphas"] == base["alphas"] == zero["alphas"] and drop39["iters"] == base["iters"]
    moved = abs(keep19["alphas"][0][0] - base["alphas"][0][0])
    assert moved > 1e4 * base["tol"]                                                  # far more than the tolerance
    g = fx["digamma"]
    xs = H.digamma_grid()
    assert g["points"] == len(xs) == len(fx["digamma_hi"]) == len(fx["digamma_lo_ulp"]) == 3576
    assert g["x_first_last"] == [xs[0], xs[-1]] and g["x_sum"] == float(np.sum(xs))
    assert 0.5 < g["scipy_worst_ulp"] < 4.0
    assert os.path.getsize(FIXTURE) < 150 * 1024


def test_definition_reproduces_the_fixture(fx, H):
    """the cheapest two cases and 200 grid points, evaluated again at 50 digits: equal to the fixture to the last stored digit"""
    pytest.importorskip("mpmath")
    for name in CHEAPEST:
        c = _case(fx, name)
        rows = H.select_rows(H.expand(H.case_table(fx, c)), c["error_filt_threshold"])
        assert len(rows) == c["kept_rows"]
        alphas, iters, margin = H.hp_fit(rows, c["max_iter"], c["tol"], c["method"])
        assert iters == c["iters"] and margin == c["margin"], name
        assert [H.split(a) for a in alphas] == c["alphas"], name
    xs = H.digamma_grid()
    pick = np.unique(np.concatenate([np.linspace(0, len(xs) - 7, 194).astype(int), np.arange(len(xs) - 6, len(xs))]))
    assert len(pick) == 200
    hi, lo = H.digamma_true(xs[pick])
    assert hi == [fx["digamma_hi"][i] for i in pick] and lo == [fx["digamma_lo_ulp"][i] for i in pick]
    below, above = fx["digamma_hi"][-2], fx["digamma_hi"][-1]
    assert below < 0.0 < above and abs(below) < 2e-16 and above < 2e-16                # either side of the root


def test_oracle_against_the_fixture_on_every_case(fx, H, oracle):
    for c in fx["cases"]:
        rows = H.expand(H.case_table(fx, c))
        got, iters = oracle.find_dirichlet_priors(rows, max_iter=c["max_iter"], tol=c["tol"], method=c["method"],
                                                  error_filt_threshold=c["error_filt_threshold"], return_iters=True)
        hi, lo = np.array(c["alphas"]).T
        err = H.rel_errors(got, hi, lo)
        print("%-22s iterations %4d  oracle error %.3g (recorded %.3g)" % (c["name"], iters, err.max(), c["oracle_rel_err"]))
        assert iters == c["iters"], c["name"]
        assert err.max() <= 2 * c["oracle_rel_err"], (c["name"], err)
        exact = (hi == 0.0) | ((hi == H.CLAMP) & (lo == 0.0)) | (c["kept_rows"] <= 5)
        assert np.array_equal(np.asarray(got)[exact], hi[exact]), c["name"]


def test_select_rows_agrees_with_the_oracle_on_the_equality_rows(fx, H, oracle):
    """rows (19, 1, 0, 0) at filter 0.05 stay (1 / 20 == 0.05, the comparison is <), rows (39, 1, 0, 0) and rows without counts go"""
    assert 1.0 / 20.0 == 0.05
    for rows, kept in (([[19, 1, 0, 0]] * 7, 7), ([[39, 1, 0, 0]] * 7, 0), ([[0, 0, 0, 0]] * 7, 0), ([[0, 19, 0, 1]] * 6 + [[1, 39, 0, 0]], 6)):
        assert len(H.select_rows(np.array(rows, float), 0.05)) == kept
        degenerate = np.array_equal(oracle.find_dirichlet_priors(np.array(rows, float), error_filt_threshold=0.05), [0, 0, 0, 1.0])
        assert degenerate == (kept <= 5)
    for name in ("base", "keep19", "drop39", "zero"):
        c = _case(fx, name + "_filter_0.05")
        rows = H.expand(H.case_table(fx, c))
        assert len(H.select_rows(rows, 0.05)) == c["kept_rows"]
        # the oracle's selection, through its result: fitting the rows select_rows keeps, without a filter, gives the same bits
        a = oracle.find_dirichlet_priors(rows, error_filt_threshold=0.05)
        b = oracle.find_dirichlet_priors(H.select_rows(rows, 0.05))
        assert np.array_equal(a, b), name
