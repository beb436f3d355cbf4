"""The Dirichlet-multinomial prior fit from its definition in high precision (mpmath), and the digamma grid with its true values.

TEST INFRASTRUCTURE ONLY: tests/golden/make_golden.py (hp-dirichlet) writes tests/golden/dirichlet_hp_golden.json with it, and
tests/test_dirichlet_hp.py recomputes a sample of that fixture.  The GPU tests (tests/test_gpu_dirichlet_hp.py) read the fixture and
use the helpers below that need no mpmath (the grid, the table expansion, the error measures); they evaluate nothing in high
precision.  mpmath is imported only inside the functions that use it.

The definition (tracs/dirichlet_multinomial.py:9-73), for a table of counts [L][K]:

    filter (:13-15)      with a threshold, cells whose count / row total < threshold become 0 (0 / 0 compares false: row unchanged)
    selection (:20-35)   rows with more than one non-zero cell are kept; with at most 5 of them the answer is (0, .., 0, 1)
    sort (:36)           every kept row ascending
    start (:40)          alpha = column means + 0.5
    FPI (:56-68)         alpha_k <- alpha_k sum_i[psi(x_ik + alpha_k) - psi(alpha_k)] / sum_i[psi(n_i + a0) - psi(a0)], a0 = sum alpha;
                         stop when sum_k |delta_k| < tol, with the new alpha as it is; otherwise clamp it at 1e-16 and go on
    LOO (:42-54)         alpha_k <- alpha_k sum_i[x_ik / (x_ik - 1 + alpha_k)] / sum_i[n_i / (n_i - 1 + a0)]; stop when max_k |delta_k| < tol
    result (:70)         sorted descending

The sums depend only on the multiset of kept rows, so they run over the distinct values of each column and the distinct totals, with
multiplicities.  A case is 'ill' when some iteration's stopping statistic D_i (sum or max of |delta|) has |D_i - tol| / tol < ILL = 1e-6:
an f64 evaluation carries about 1e-14 relative error in D, so outside that margin it stops at the same iteration as the definition.
The fixture holds no ill case.
"""
import math

import numpy as np

DPS = 50
ILL = 1e-6
CLAMP = 1e-16

# ---- the digamma grid: plain float arithmetic only (products, sums and one quotient of doubles), the same on every machine ------------
_R_SMALL = 1.1311278765939214          # 10 ** (16 / 299): 300 points from 1e-16 to 1 (the last is 1 - 4e-15)
_R_LARGE = 1.1030586363657415          # (3e8) ** (1 / 199): 200 points from 10 to 3e9
ROOT_BELOW = 1.4616321449683622        # psi < 0 here and > 0 at the next double: the root is 1.46163214496836234126...


def digamma_grid():
    """-> float64[3576]: 300 log-spaced in [1e-16, 1], 3000 evenly spaced in [0.01, 12], 200 log-spaced in [10, 3e9], the
    half-integers 0.5 .. 69.5, then 1, 2, 6, 10 and the two doubles either side of the root"""
    xs, x = [], 1e-16
    for _ in range(300):
        xs.append(x)
        x *= _R_SMALL
    step = (12.0 - 0.01) / 2999.0
    xs += [0.01 + i * step for i in range(3000)]
    x = 10.0
    for _ in range(200):
        xs.append(x)
        x *= _R_LARGE
    xs += [0.5 + i for i in range(70)]
    xs += [1.0, 2.0, 6.0, 10.0, ROOT_BELOW, math.nextafter(ROOT_BELOW, 2.0)]
    return np.array(xs, np.float64)


def ulp_errors(got, hi, lo):
    """(got - true) in units of ulp(max(|true|, 1)), true = hi + lo (hi the nearest double, lo the double of the remainder)"""
    got, hi, lo = (np.asarray(a, np.float64) for a in (got, hi, lo))
    return ((got - hi) - lo) / np.spacing(np.maximum(np.abs(hi), 1.0))


def rel_errors(got, hi, lo):
    """|got - true| / |true| per alpha, true = hi + lo; 0 where both are exactly equal (the exact 0 and 1e-16 alphas included)"""
    got, hi, lo = (np.asarray(a, np.float64) for a in (got, hi, lo))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs((got - hi) - lo) / np.abs(hi)
    return np.where((got == hi) & (lo == 0.0), 0.0, e)


def expand(table):
    """[[c_0, .., c_{K-1}, multiplicity], ..] -> float64[M][K], every distinct row repeated, in the table's order"""
    t = np.asarray(table, np.float64)
    return np.repeat(t[:, :-1], t[:, -1].astype(np.int64), axis=0)


def case_table(fx, case):
    """the rows of a fixture case: its table, plus the case's own extra rows (the filter variants add one row to a shared table)"""
    return fx["tables"][case["table"]] + case.get("extra_rows", [])


def distinct(rows):
    """float rows [M][K] -> [[c_0, .., c_{K-1}, multiplicity], ..] of ints, in order of first appearance"""
    seen = {}
    for r in np.asarray(rows).astype(np.int64).tolist():
        seen[tuple(r)] = seen.get(tuple(r), 0) + 1
    return [list(r) + [m] for r, m in seen.items()]


def select_rows(counts, error_filt_threshold=None):
    """the filter and the selection (:13-35) in doubles, as the reference does them -> the kept rows, unsorted, in site order"""
    x = np.array(counts, dtype=np.float64)
    if error_filt_threshold is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            freq = (x.T / np.sum(x, 1)).T                      # 0 / 0 = nan compares false: the row stays as it is
        x[freq < error_filt_threshold] = 0
    return x[np.count_nonzero(x, 1) > 1]


# ---- high precision ------------------------------------------------------------------------------------------------------------------
def split(v):
    """mpf -> [nearest double, double of the remainder]: resolves the value to about 1e-32 relative"""
    from mpmath import mpf
    hi = float(v)
    return [hi, float(v - mpf(hi))]


def digamma_true(xs):
    """-> (hi[], lo[]) of psi(x) at DPS digits for the exact values of the doubles xs: the nearest double, and the remainder in units
    of ulp(hi)"""
    from mpmath import mp, mpf
    hi, lo = [], []
    with mp.workdps(DPS):
        for x in xs:
            h, l = split(mp.digamma(mpf(float(x))))
            hi.append(h)
            lo.append(round(l / float(np.spacing(abs(h))), 4))  # in ulp(hi), to 1e-4: far below the 0.01 ulp a test needs
    return hi, lo


def digamma_lo(hi, lo_ulp):
    """the remainders as doubles, from their stored form (units of ulp(hi))"""
    hi = np.asarray(hi, np.float64)
    return np.asarray(lo_ulp, np.float64) * np.spacing(np.abs(hi))


def _weighted(values, mult):
    from mpmath import mpf
    u, inv = np.unique(values, return_inverse=True)
    c = np.bincount(inv.ravel(), weights=mult).astype(np.int64)
    return [(mpf(float(v)), int(n)) for v, n in zip(u, c)]


def hp_fit(rows, max_iter=1000, tol=1e-5, method="FPI", mult=None):
    """The fit of the kept `rows` (float [M][K], M > 5; mult: multiplicity of each row, default 1) at DPS digits
    -> (alphas descending as mpf, iterations done, min_i |D_i - tol| / tol over the iterations done or None when there was none)"""
    from mpmath import mp, mpf
    x = np.sort(np.asarray(rows, np.float64), axis=1)                                       # :36
    M, K = x.shape
    mult = np.ones(M, np.int64) if mult is None else np.asarray(mult, np.int64)
    assert int(mult.sum()) > 5
    with mp.workdps(DPS):
        cols = [_weighted(x[:, k], mult) for k in range(K)]
        tots = _weighted(x.sum(1), mult)                                                    # sums of integers below 2^53: exact
        n = int(mult.sum())
        alpha = [sum(v * c for v, c in cols[k]) / n + mpf(0.5) for k in range(K)]           # :40
        T, floor = mpf(float(tol)), mpf(CLAMP)
        iters, margin = 0, None
        for _ in range(int(max_iter)):
            a0 = sum(alpha)
            if method == "LOO":                                                             # :43-54
                den = sum(c * t / (t - 1 + a0) for t, c in tots)
                new = [alpha[k] * sum(c * v / (v - 1 + alpha[k]) for v, c in cols[k] if v != 0) / den for k in range(K)]
                stat = max(abs(b - a) for a, b in zip(alpha, new))
                conv = stat < T
                alpha = new
            else:                                                                           # :56-68
                p0 = mp.digamma(a0)
                den = sum(c * (mp.digamma(t + a0) - p0) for t, c in tots)
                new = []
                for k in range(K):
                    pk = mp.digamma(alpha[k])
                    new.append(alpha[k] * sum(c * (mp.digamma(v + alpha[k]) - pk) for v, c in cols[k] if v != 0) / den)
                stat = sum(abs(b - a) for a, b in zip(alpha, new))
                conv = stat < T
                alpha = new if conv else [max(a, floor) for a in new]
            iters += 1
            m = float(abs(stat - T) / T)
            margin = m if margin is None else min(margin, m)
            if conv:
                break
        return sorted(alpha, reverse=True), iters, margin                                   # :70
