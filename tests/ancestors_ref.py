"""CPU reference for `tracs distance --ancestors`, written from its definition: sample a is a candidate source of sample s when
{a, s} is an eligible pair and a's day is strictly earlier; the chosen source is the smallest candidate under (value key, day gap,
index of a).  kind 0: integer values ascending; 1: f64 ascending; 2: f64 descending; f64 values compare as numbers, -0.0 equals +0.0
and every NaN sorts after every number in either direction."""
import numpy as np


def value_key(value, kind):
    """-> (nan flag, number) whose lexicographic order is the value order of `kind`."""
    v = np.asarray(value)
    if kind == 0:
        return np.zeros(len(v), bool), v.astype(np.int64)
    v = v.astype(np.float64)
    nan = np.isnan(v)
    num = np.where(nan, 0.0, v) + 0.0                     # -0.0 + 0.0 == +0.0: the two zeros tie
    return nan, (num if kind == 1 else -num + 0.0)


def ancestors(n, days, i, j, value, kind, eligible=None):
    """-> (parent, edge): per sample its chosen source and the position of the chosen pair among (i, j, value); -1 for a root.
    Pairs come in either order and must be unique; a loop, an endpoint outside [0, n) or a pair with equal days is no candidate."""
    days = np.asarray(days, np.int64)
    i = np.asarray(i, np.int64)
    j = np.asarray(j, np.int64)
    ok = (i != j) & (i >= 0) & (j >= 0) & (i < n) & (j < n)
    if eligible is not None:
        ok &= np.asarray(eligible, bool)
    ii, jj = np.where(ok, i, 0), np.where(ok, j, 0)
    ok &= days[ii] != days[jj]
    pos = np.flatnonzero(ok)
    i_later = days[i[pos]] > days[j[pos]]
    s = np.where(i_later, i[pos], j[pos])
    a = np.where(i_later, j[pos], i[pos])
    gap = days[s] - days[a]
    nan, num = value_key(np.asarray(value)[pos], kind)
    order = np.lexsort((a, gap, num, nan, s))
    parent = np.full(n, -1, np.int64)
    edge = np.full(n, -1, np.int64)
    if len(order):
        so = s[order]
        first = np.ones(len(so), bool)
        first[1:] = so[1:] != so[:-1]
        parent[so[first]] = a[order][first]
        edge[so[first]] = pos[order][first]
    return parent, edge


def brute_force(n, days, i, j, value, kind, eligible=None):
    """The same by the definition's words: per sample, a loop over every pair (tests check `ancestors` against it)."""
    import math

    def vkey(x):
        if kind == 0:
            return (0, int(x))
        x = float(x)
        if math.isnan(x):
            return (1, 0.0)
        x = 0.0 if x == 0.0 else x
        return (0, x if kind == 1 else -x)
    parent, edge = [-1] * n, [-1] * n
    for s in range(n):
        best = None
        for e in range(len(i)):
            if eligible is not None and not eligible[e]:
                continue
            x, y = int(i[e]), int(j[e])
            if x == y or not (0 <= x < n and 0 <= y < n) or s not in (x, y):
                continue
            a = y if x == s else x
            if not days[a] < days[s]:
                continue
            k = (vkey(value[e]), int(days[s]) - int(days[a]), a)
            if best is None or k < best[0]:
                best = (k, a, e)
        if best is not None:
            parent[s], edge[s] = best[1], best[2]
    return np.array(parent, np.int64), np.array(edge, np.int64)


def trees(parent):
    """-> (root, generation) per sample: the sample reached by following sources, and the number of links to it."""
    parent = np.asarray(parent, np.int64)
    n = len(parent)
    root = np.full(n, -1, np.int64)
    gen = np.zeros(n, np.int64)
    for v in range(n):
        path = []
        x = v
        while root[x] < 0 and parent[x] >= 0:
            path.append(x)
            x = int(parent[x])
            assert len(path) <= n, "cycle"
        if root[x] < 0:
            root[x], gen[x] = x, 0
        r, g = root[x], gen[x]
        for y in reversed(path):
            g += 1
            root[y], gen[y] = r, g
    return root, gen


def links(parent, edge):
    """Positions of the chosen pairs in (min, max) order of their samples -- the order of the output rows."""
    parent = np.asarray(parent, np.int64)
    s = np.flatnonzero(parent >= 0)
    lo, hi = np.minimum(s, parent[s]), np.maximum(s, parent[s])
    o = np.lexsort((hi, lo))
    return np.asarray(edge, np.int64)[s[o]], lo[o], hi[o]
