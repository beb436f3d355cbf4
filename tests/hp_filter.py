"""The recombination filter's keep / drop decision from its definition in high precision (mpmath), and crafted SNP positions that
make the filter decide the cells on either side of that boundary.

TEST INFRASTRUCTURE ONLY: tests/golden/make_golden.py (hp-filter) writes tests/golden/filter_hp_golden.json with it, and
tests/test_filter_hp.py recomputes a sample of that fixture.  The GPU tests (tests/test_gpu_filter_hp.py) read the fixture and
use the builder of positions; they evaluate nothing in high precision.

The definition (src/pairsnp.hpp filter_recomb :251-318, range_count :223-248, cached_binomial_cdf :41-58), for a pair with d > 1 SNPs
in an alignment of L sites:

    p = d / L    thr = 0.05 / d    wh = clamp(int(1.0 / p / 2.0 + 1), 50, 5000)                  (doubles: Python floats)

and every SNP at site i looks at the window [max(0, i - wh), min(L, i + wh + 1)): with `count` SNPs inside, spanning `length` sites
from the first to the last of them, the SNP is kept when count <= 1 or

    tail = 1 - CDF(count; length, p) = P(X > count),  X ~ Binomial(length, p),      tail >= thr,

where CDF = 1 (tail = 0: dropped) for count >= length.  The filtered distance is the number of SNPs kept.

A cell (count, length) is 'ill' when |tail - thr| <= MARGIN thr, MARGIN = 1e-9: a double evaluation of 1 - cdf carries about 1e-16
absolute error (cdf is near 1), which is 1.6e-10 of the smallest threshold a table row has (0.05 / 65 536 = 7.6e-7), and MARGIN
leaves some room above that.  Outside the margin a careful double evaluation decides as the definition does; the fixture's cases
hold no ill cell.
"""
import numpy as np
from mpmath import mp, mpf

DPS = 50
MARGIN = 1e-9
K_LO, K_HI = 2, 63                     # the counts that have a column in the device's threshold rows
K_BIG = 64                             # the first count without one
RUN = 4                                # a run of consecutive SNPs: count == length
ORDER = (2, 3, 5, 9, 17, "run", 40, 63, "big") + tuple(k for k in range(K_LO, K_HI + 1) if k not in (2, 3, 5, 9, 17, 40, 63))


def window(L, d):
    """-> (p, thr, wh) as the reference's doubles"""
    p = float(d) / int(L)
    thr = 0.05 / float(d)
    wh = int(1.0 / p / 2.0 + 1)
    wh = max(min(wh, 5000), 50)
    return p, thr, wh


_tails = {}


def tail(n, k, p):
    """P(X > k), X ~ Binomial(n, p) with p the exact value of that double: the exact terms summed on the shorter side (mpf)"""
    n, k = int(n), int(k)
    key = (n, k, float(p))
    if key in _tails:
        return _tails[key]
    with mp.workdps(DPS):
        if k >= n:
            t = mpf(0)
        else:
            P = mpf(float(p))
            Q = 1 - P
            if n - k <= k + 1:                     # upper side: j = n down to k + 1
                term = P ** n
                s = term
                for j in range(n, k + 1, -1):      # term(j - 1) = term(j) j / (n - j + 1) Q / P
                    term = term * j / (n - j + 1) * Q / P
                    s += term
                t = s
            else:                                  # lower side: j = 0 .. k
                term = Q ** n
                s = term
                for j in range(k):                 # term(j + 1) = term(j) (n - j) / (j + 1) P / Q
                    term = term * (n - j) / (j + 1) * P / Q
                    s += term
                t = 1 - s
    _tails[key] = t
    return t


def rel_margin(n, k, L, d):
    """|tail - thr| / thr of one cell, as a float"""
    p, thr, _ = window(L, d)
    with mp.workdps(DPS):
        return float(abs(tail(n, k, p) - mpf(thr)) / mpf(thr))


def classify(n, k, L, d):
    """'keep', 'drop' or 'ill' for a window of k (> 1) SNPs spanning n sites"""
    p, thr, _ = window(L, d)
    with mp.workdps(DPS):
        t, T = tail(n, k, p), mpf(thr)
        if abs(t - T) <= mpf(MARGIN) * T:
            return "ill"
        return "keep" if t >= T else "drop"


def n_star(L, d, k):
    """the smallest n in (k, min(L, 2 wh + 1)] with tail >= thr, or None: located in double, both neighbours confirmed at DPS digits"""
    from scipy.stats import binom
    p, thr, wh = window(L, d)
    hi = min(int(L), 2 * wh + 1)
    lo = k + 1
    if lo > hi:
        return None
    if classify(hi, k, L, d) != "keep":
        assert classify(hi, k, L, d) == "drop", ("ill at the widest span", L, d, k)
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if binom.sf(k, mid, p) >= thr:
            hi = mid
        else:
            lo = mid + 1
    n = lo
    while n > k + 1 and classify(n - 1, k, L, d) != "drop":      # the double search may be off next to the boundary
        n -= 1
    while classify(n, k, L, d) == "drop":
        n += 1
    # the tail grows with n: keep at n*, drop at n* - 1, neither inside the margin
    assert classify(n, k, L, d) == "keep" and (n - 1 == k or classify(n - 1, k, L, d) == "drop"), (L, d, k, n)
    assert tail(n, k, p) > tail(n - 1, k, p)
    return n


def row(L, d):
    """[n*(k) for k = 2 .. 63], None where no window of the pair can survive with k SNPs"""
    return [n_star(L, d, k) for k in range(K_LO, K_HI + 1)]


def filter_positions(pos, L):
    """filter_recomb over the sorted SNP sites of one pair -> (kept, {(count, length): kept?} of the windows with count > 1,
    number of ill cells among them, smallest |tail - thr| / thr among them (1.0 when there is none))"""
    pos = np.asarray(pos, np.int64)
    d = len(pos)
    if d <= 1:
        return d, {}, 0, 1.0
    assert (np.diff(pos) > 0).all() and pos[0] >= 0 and pos[-1] < L
    p, thr, wh = window(L, d)
    lo = np.searchsorted(pos, np.maximum(0, pos - wh), "left")
    hi = np.searchsorted(pos, np.minimum(L, pos + wh + 1), "left")
    count = hi - lo
    length = pos[hi - 1] - pos[lo] + 1
    kept = int((count <= 1).sum())
    cells, ill, margin = {}, 0, 1.0
    multi = count > 1
    if not multi.any():
        return kept, cells, ill, margin
    uniq, times = np.unique(np.stack([count[multi], length[multi]], 1), axis=0, return_counts=True)
    for (k, n), m in zip(uniq.tolist(), times.tolist()):
        c = classify(n, k, L, d)
        ill += c == "ill"
        margin = min(margin, rel_margin(n, k, L, d))
        cells[(k, n)] = c == "keep"
        if c == "keep":
            kept += m
    return kept, cells, ill, margin


# ---- crafted positions -------------------------------------------------------------------------------------------------------------
def _cluster(first, k, span):
    """k sites over exactly `span`: the first, the last, the centre first + (span - 1) // 2 and the rest next to the centre"""
    last, c = first + span - 1, first + (span - 1) // 2
    assert k <= span and k >= 2
    s = {first, last}
    if k > 2:
        s.add(c)
    off = 1
    while len(s) < k:
        for x in (c + off, c - off):
            if first < x < last and len(s) < k:
                s.add(x)
        off += 1
    return sorted(s)


def _mix(x):
    """splitmix64 of a uint64 array: the seeded choice of filler sites, the same on every machine and library version"""
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def plan(L, d, row):
    """-> (sorted sites, the k whose two boundary cells (k, n*) and (k, n* - 1) the sites make the filter decide)

    Clusters in the order ORDER, as many as fit d SNPs and half the alignment: for a k with n* = row[k - 2] one cluster of k SNPs
    spanning n* and one spanning n* - 1 (attainable when n* <= 2 wh + 1; k = 2: n* <= wh + 1, the two ends must see each other); for
    a k without, one cluster at the widest attainable span; 'run': RUN consecutive sites; 'big': K_BIG SNPs at the widest span.
    The first cluster starts at site 0 and the last one placed ends at L - 1; every cluster is wh + 1 sites from any other SNP.
    Fillers make up d: wh + 1 apart where there is room, at seeded sites of the free stretch otherwise."""
    L, d = int(L), int(d)
    _, _, wh = window(L, d)
    widest = min(L, 2 * wh + 1)
    gap = wh + 1

    def fits(cl):
        used = sum(k for k, _ in cl)
        if used > d:
            return False
        foot = sum(s + gap for _, s in cl)
        if len(cl) > 1 and foot > L // 2:
            return False
        if len(cl) == 1:
            return cl[0][1] <= L if used == d else cl[0][1] + gap + 3 * (d - used) <= L
        return L - foot - gap + 1 >= 3 * (d - used)

    clusters, covered = [], []
    for item in ORDER:
        if item == "run":
            new = [(RUN, RUN)]
        elif item == "big":
            new = [(K_BIG, widest)] if widest >= K_BIG else []
        else:
            k, ns = item, row[item - K_LO]
            top = min(wh + 1, widest) if k == 2 else widest
            if ns is None or ns > top:
                new = [(k, top)] if top >= k else []
            else:
                new = [(k, ns), (k, ns - 1)]
        if not new:
            continue
        if fits(clusters + new):
            clusters += new
            if len(new) == 2:
                covered.append(item)
        else:
            if len(new) == 2 and fits(clusters + new[:1]):
                clusters += new[:1]
            break
    sites, at = [], 0
    for i, (k, s) in enumerate(clusters):
        if i == len(clusters) - 1 and i > 0:
            break
        sites += _cluster(at, k, s)
        at += s + gap
    a, b = at, L - 1
    if len(clusters) > 1:
        k, s = clusters[-1]
        sites += _cluster(L - s, k, s)
        b = L - s - gap
    m = d - len(sites)
    if m > 0:
        assert b - a + 1 >= m, (L, d, a, b, m)
        if (m - 1) * gap <= b - a:
            step = (b - a) // max(m - 1, 1) if m > 1 else 0
            sites += [a + j * step for j in range(m)]
        else:
            key = _mix(np.arange(a, b + 1, dtype=np.uint64) + np.uint64(L) * np.uint64(1000003) + np.uint64(d))
            sites += (a + np.sort(np.argsort(key, kind="stable")[:m])).tolist()
    sites = sorted(sites)
    assert len(sites) == d and len(set(sites)) == d and sites[0] >= 0 and sites[-1] < L, (L, d, len(sites))
    return sites, covered


def boundary_positions(L, d, row):
    """exactly d distinct sorted sites in [0, L) whose windows hold the boundary cells of `row` (see plan)"""
    return plan(L, d, row)[0]


def must_hit(L, d, row):
    """the cells the sites of boundary_positions are built to make the filter decide: (k, n*) and (k, n* - 1) of every covered k"""
    return [(k, row[k - K_LO] - e) for k in plan(L, d, row)[1] for e in (0, 1)]


# ---- probes of the half window -----------------------------------------------------------------------------------------------------
PROBES = ("pair", "far2")


def probe_positions(L, d, shape, gap):
    """d sorted sites: one SNP at site 0, one `gap` sites on ('far2': and one just before that), and the other SNPs evenly spread
    over the rest of the alignment, out of sight of these (the same sites for gap = wh and gap = wh + 1).  At gap = wh the
    first and the last of the probe see each other, at wh + 1 they do not: a pair of SNPs against two singletons, or, where the
    filter keeps such a pair, three SNPs over wh + 1 sites against two over wh + 1 and two over 2."""
    head = [0, gap] if shape == "pair" else [0, gap - 1, gap]
    rest = d - len(head)
    assert rest >= 0
    _, _, wh = window(L, d)
    start = 2 * wh + 4
    step = (L - start) // max(rest, 1)
    assert rest == 0 or step >= 1, (L, d)
    return head + [start + j * step for j in range(rest)]


def choose_probe(L, d):
    """-> (shape, kept at gap wh, kept at gap wh + 1) of the first shape for which the two differ, and no cell is ill"""
    _, _, wh = window(L, d)
    for shape in PROBES:
        if d < (2 if shape == "pair" else 3):
            continue
        a = filter_positions(probe_positions(L, d, shape, wh), L)
        b = filter_positions(probe_positions(L, d, shape, wh + 1), L)
        if a[0] != b[0] and a[2] == 0 and b[2] == 0:
            return shape, a[0], b[0]
    raise AssertionError(("no probe tells wh from wh + 1", L, d))
