"""The recombination filter on the tree's branches, restated in plain Python: the reference of tracs_fitch_edge_sites,
tracs_filter_recomb_lists and `tracs distance --tree nj --tree-filter`.

fitch_ref.fitch's entries regrouped by edge give C_e, the ascending sites with a change on edge e; kept_e is
oracle.filter_recomb_positions(C_e, L).  verdicts() restates the window test once more per entry (with oracle.binomial_cdf for the
tail), for the `dropped` flags and for the margin of the seeded inputs: windows() gives the (count, length) of the windows a list makes the
filter decide, and margin() how far the nearest one is from its threshold.

TEST INFRASTRUCTURE ONLY.  The seeded lists of the GPU tests are defined here (own_edge_cases), so that the CPU test of their
margin and the GPU tests read the same inputs.
"""
import numpy as np

import fitch_ref

MARGIN = 1e-9


def edge_lists(parent, child, masks):
    """-> (fitch_ref.fitch's dict, [ascending sites with a change on edge e] for every edge)"""
    r = fitch_ref.fitch(parent, child, masks)
    lists = [[] for _ in range(len(parent))]
    for s, e, _ in r["entries"]:                                   # (sites ascending: every list comes out ascending)
        lists[e].append(s)
    return r, [np.asarray(x, np.int64) for x in lists]


def flat(lists):
    """-> (off int64 [m + 1], pos int64) of a list of lists"""
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    pos = np.concatenate([np.asarray(x, np.int64) for x in lists]) if len(lists) and off[-1] else np.zeros(0, np.int64)
    return off, pos


def window(L, d):
    p = float(d) / int(L)
    thr = 0.05 / float(d)
    wh = max(min(int(1.0 / p / 2.0 + 1), 5000), 50)
    return p, thr, wh


def windows(pos, L):
    """-> (count, length) of every entry's window, as arrays"""
    pos = np.asarray(pos, np.int64)
    _, _, wh = window(L, len(pos))
    lo = np.searchsorted(pos, np.maximum(0, pos - wh), "left")
    hi = np.searchsorted(pos, np.minimum(L, pos + wh + 1), "left")
    return hi - lo, pos[hi - 1] - pos[lo] + 1


def verdicts(pos, L, oracle):
    """-> bool array: kept?  per entry of one ascending list"""
    pos = np.asarray(pos, np.int64)
    d = len(pos)
    if d <= 1:
        return np.ones(d, bool)
    p, thr, _ = window(L, d)
    count, length = windows(pos, L)
    keep = {}
    for k, n in set(zip(count.tolist(), length.tolist())):
        keep[(k, n)] = True if k <= 1 else (1.0 - oracle.binomial_cdf(n, p, k)) >= thr
    return np.array([keep[c] for c in zip(count.tolist(), length.tolist())], bool)


def margin(pos, L, oracle):
    """the smallest |tail - thr| / thr over the windows with count > 1 of one list (1.0 where there is none)"""
    pos = np.asarray(pos, np.int64)
    d = len(pos)
    if d <= 1:
        return 1.0
    p, thr, _ = window(L, d)
    count, length = windows(pos, L)
    best = 1.0
    for k, n in set(zip(count.tolist(), length.tolist())):
        if k > 1:
            best = min(best, abs((1.0 - oracle.binomial_cdf(n, p, k)) - thr) / thr)
    return best


def branch_filter(parent, child, masks, oracle):
    """-> (fitch dict, lists, kept per edge)"""
    r, lists = edge_lists(parent, child, masks)
    L = np.asarray(masks).shape[1]
    return r, lists, np.array([oracle.filter_recomb_positions(x, L) for x in lists], np.int64)


# ---- the seeded lists of tests/test_gpu_branch_filter.py ---------------------------------------------------------------------------
def _draw(rng, L, d):
    return np.sort(rng.choice(L, d, replace=False)).astype(np.int64)


def _clustered(rng, L, d, centres, width):
    """d distinct sites: half of them uniform, half within `width` of one of a few centres"""
    c = rng.integers(0, L, centres)
    near = np.clip(c[rng.integers(0, centres, 4 * d)] + rng.integers(-width, width + 1, 4 * d), 0, L - 1)
    got = np.unique(np.concatenate([rng.choice(L, d // 2, replace=False), near]))
    rng.shuffle(got)
    return np.sort(got[:d]).astype(np.int64)


def own_edge_cases():
    """[(name, L, [ascending int64 lists])]: the seeds were chosen so that no window lies within MARGIN of its threshold
    (tests/test_branch_filter_ref.py checks every one of them; a seed that fails there is replaced, never tolerated)"""
    cases = []
    rng = np.random.default_rng(2101)
    L = 5000
    e = np.zeros(0, np.int64)
    # empty lists between non-empty ones, d = 1, d = 2 (seeing each other and not), the two ends of the alignment
    cases.append(("empties, d = 1, d = 2, both ends", L,
                  [e, np.array([17]), e, e, np.array([100, 130]), np.array([100, 4000]), e, np.array([0, L - 1]), np.array([0]),
                   np.array([L - 1]), np.array([0, 1, L - 2, L - 1]), e, _draw(rng, L, 40), e]))
    # runs of adjacent sites: count >= length
    cases.append(("runs of adjacent sites", L,
                  [np.arange(200, 204), np.concatenate([np.arange(0, 6), _draw(rng, L - 200, 30) + 100, np.arange(L - 5, L)]),
                   np.arange(1000, 1100)]))
    # a window with >= 64 changes: beyond the threshold rows' counts
    dense = np.unique(np.concatenate([np.arange(3000, 3400, 3), _draw(rng, 50000, 300)]))
    cases.append(("a window with more than 63 changes", 50000, [dense, _clustered(rng, 50000, 500, 3, 40)]))
    # random and clustered lists of many lengths around the half window's clamps
    L = 30000
    cases.append(("random and clustered", L,
                  [_draw(rng, L, d) for d in (2, 3, 5, 9, 33, 64, 65, 129, 700)] + [_clustered(rng, L, d, 4, 25) for d in (12, 60, 300, 2000)]))
    # one list beyond the rows' d (FLT_DCAP = 65 536) next to a thousand short ones
    L = 200000
    rng = np.random.default_rng(2202)
    cases.append(("70 000 entries next to 1 000 lists of 3", L,
                  [_draw(rng, L, 3) for _ in range(500)] + [_draw(rng, L, 70000)] + [_clustered(rng, L, 3, 1, 30) for _ in range(500)]))
    cases.append(("L = 1", 1, [e, np.array([0]), e, np.array([0])]))
    return cases


def tree_case():
    """-> (masks, parent, child) of nine samples on a seeded tree with an import on one terminal branch: the input of the marked-entries
    test (its margin is checked with the lists above)"""
    rng = np.random.default_rng(77)
    n, L = 9, 6000
    base = rng.integers(0, 4, L)
    seqs = np.where(rng.random((n, L)) < 0.01, rng.integers(0, 4, (n, L)), base)
    seqs[3, 2000:2030] = (base[2000:2030] + 1) % 4
    parent, child = fitch_ref.random_tree(n, rng)
    return (1 << seqs).astype(np.int64), parent, child
