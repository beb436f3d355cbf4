"""CPU reference for `tracs distance --mst`: Kruskal under the order (weight, i, j), i < j, which makes the minimum spanning forest
unique.  f64 weights compare as numbers, -0.0 equals +0.0 and every NaN sorts above +inf (csrc/forest.hip's key)."""
import numpy as np


def order(i, j, w):
    """Edge positions sorted by (weight, min(i, j), max(i, j))."""
    i = np.asarray(i, np.int64)
    j = np.asarray(j, np.int64)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    w = np.asarray(w)
    if w.dtype.kind == "f":
        w = w.astype(np.float64)
        nan = np.isnan(w)
        val = np.where(nan, 0.0, w) + 0.0                 # -0.0 + 0.0 == +0.0: the two zeros tie
        return np.lexsort((hi, lo, val, nan))
    return np.lexsort((hi, lo, w.astype(np.int64)))


def forest(n, i, j, w):
    """Positions of the forest's edges among (i, j, w), in (min, max) order.  Pairs must be unique and i != j."""
    i = np.asarray(i, np.int64)
    j = np.asarray(j, np.int64)
    parent = list(range(int(n)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    chosen = []
    need = int(n) - 1
    for e in order(i, j, w).tolist():
        a, b = find(int(i[e])), find(int(j[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            chosen.append(e)
            if len(chosen) == need:
                break
    chosen = np.asarray(chosen, np.int64)
    lo, hi = np.minimum(i[chosen], j[chosen]), np.maximum(i[chosen], j[chosen])
    return chosen[np.lexsort((hi, lo))]


def partition(n, i, j):
    """Connected components of the graph on [0, n) as a set of frozensets, isolated vertices left out (they are in no row)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    i = np.asarray(i, np.int64)
    j = np.asarray(j, np.int64)
    g = sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(n, n)).tocsr()
    _, lab = connected_components(g, directed=False)
    seen = np.zeros(n, bool)
    seen[i] = True
    seen[j] = True
    groups = {}
    for v in np.flatnonzero(seen).tolist():
        groups.setdefault(int(lab[v]), set()).add(v)
    return {frozenset(s) for s in groups.values()}


def threshold_partition(n, i, j, w, t):
    """The components that `cluster -c t` forms from the rows (i, j, w): edges with w <= t (a NaN never), every row's samples."""
    i = np.asarray(i, np.int64)
    j = np.asarray(j, np.int64)
    keep = np.asarray(w, np.float64) <= t
    base = partition(n, np.concatenate([i[keep], i, j]), np.concatenate([j[keep], i, j]))
    return base
