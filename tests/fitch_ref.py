"""Small parsimony on a fixed tree, restated in plain Python / numpy: the reference of tracs_fitch_count / _fill.

Input: masks, an n x L array of allele sets (A = 1, C = 2, G = 4, T = 8, never 0, N = 15), and the tree exactly as tracs_nj_edges
returns it: 2n - 3 edges in creation order, (n + t, a_t), (n + t, b_t) with a_t < b_t for join t = 0 .. n - 4, then the top node
T = 2n - 3 with x < y < z.  Sites are independent.

Bottom-up, ascending node id.  S_i = m_i for a leaf.  Join t: I = S_a & S_b; non-zero: S_{n+t} = I, else S_{n+t} = S_a | S_b and the
cost rises by 1.  Top node: S_xy from S_x and S_y by the same rule (same cost), then I = S_xy & S_z; non-zero: S_T = I, else S_T = S_xy
and the cost rises by 1.

Top-down.  lowbit(m) = m & -m.  f_T = lowbit(S_T); the edges by descending parent id, creation order within a parent;
f_child = f_parent if f_parent & S_child != 0, else lowbit(S_child).  A change is an edge with f_child != f_parent.

n = 1: no edge, no change.  n = 2: the edge (0, 1); f_0 = lowbit(m_0 & m_1), or lowbit(m_0) if that is zero; f_1 by the child rule.

minimum(s) = (the smallest |H|, H a non-empty set of bases with m_i(s) & H != 0 for every i) - 1.
"""
import itertools

import numpy as np


def lowbit(m):
    return m & -m


def walk_order(n, n_edges):
    """the edge indices in the order of the top-down walk"""
    if n < 3:
        return list(range(n_edges))
    J = n - 3
    order = [2 * J, 2 * J + 1, 2 * J + 2]
    for t in range(J - 1, -1, -1):
        order += [2 * t, 2 * t + 1]
    return order


def fitch(parent, child, masks):
    """-> dict: edge_changes [n_edges], site_changes [L], site_cost [L] (the bottom-up cost), site_minimum [L], off [L + 1], total,
    entries = [(site, edge, info)] sites ascending and walk order within a site, info = f_parent | f_child << 4.  Every step is the
    definition's, applied to all sites at once (the sites are independent)."""
    masks = np.asarray(masks, dtype=np.int64)
    n, L = masks.shape
    parent = [int(x) for x in parent]
    child = [int(x) for x in child]
    ne = len(parent)
    assert ne == (2 * n - 3 if n >= 3 else n - 1)
    edge_changes = np.zeros(ne, np.int64)
    site_changes = np.zeros(L, np.int64)
    cost = np.zeros(L, np.int64)
    S = {i: masks[i] for i in range(n)}

    def join(a, b):
        i = a & b
        empty = i == 0
        return np.where(empty, a | b, i), empty.astype(np.int64)

    f = {}
    if n == 2:
        assert (parent[0], child[0]) == (0, 1)
        i = masks[0] & masks[1]
        cost += i == 0
        f[0] = lowbit(np.where(i == 0, masks[0], i))
    elif n >= 3:
        J = n - 3
        for t in range(J):
            assert parent[2 * t] == parent[2 * t + 1] == n + t and child[2 * t] < child[2 * t + 1]
            S[n + t], c = join(S[child[2 * t]], S[child[2 * t + 1]])
            cost += c
        x, y, z = child[2 * J:2 * J + 3]
        assert x < y < z and parent[2 * J] == parent[2 * J + 1] == parent[2 * J + 2] == 2 * n - 3
        sxy, c = join(S[x], S[y])
        cost += c
        i = sxy & S[z]
        cost += i == 0
        S[2 * n - 3] = np.where(i == 0, sxy, i)
        f[2 * n - 3] = lowbit(S[2 * n - 3])
    found = []                                     # (site, rank in the walk, edge, info) of every change
    for rank, e in enumerate(walk_order(n, ne)):
        p, c = parent[e], child[e]
        f[c] = np.where(f[p] & S[c], f[p], lowbit(S[c]))
        at = np.flatnonzero(f[c] != f[p])
        edge_changes[e] = len(at)
        site_changes[at] += 1
        found += [(int(s), rank, e, int(f[p][s] | (f[c][s] << 4))) for s in at]
    found.sort()
    off = np.zeros(L + 1, np.int64)
    np.cumsum(site_changes, out=off[1:])
    return {"edge_changes": edge_changes, "site_changes": site_changes, "site_cost": cost, "site_minimum": minimum(masks),
            "off": off, "total": int(off[L]), "entries": [(s, e, info) for s, _, e, info in found]}


def minimum(masks):
    """per site: (the smallest |H| with m_i & H != 0 for every sample i) - 1, by enumeration of the 15 sets"""
    masks = np.asarray(masks, dtype=np.int64)
    n, L = masks.shape
    best = np.full(L, 4, np.int64)
    for H in range(1, 16):
        hits_all = ((masks & H) != 0).all(axis=0)
        best = np.where(hits_all, np.minimum(best, bin(H).count("1")), best)
    return best - 1


def exhaustive_minimum(parent, child, column):
    """One site: the fewest edges with different end states over ALL assignments of a base to every node with leaf i's base in
    column[i] (small n only).  Every assignment of the internal nodes is tried; a leaf hangs on one edge only, so its best base
    given its parent's is known: the parent's when its mask has it (no change), else any of its own (one change)."""
    n = len(column)
    parent = [int(x) for x in parent]
    child = [int(x) for x in child]
    if n == 1:
        return 0
    if n == 2:
        return 0 if int(column[0]) & int(column[1]) else 1
    best = None
    for states in itertools.product((1, 2, 4, 8), repeat=n - 2):
        c = 0
        for p, q in zip(parent, child):
            if q >= n:
                c += states[p - n] != states[q - n]
            else:
                c += not (states[p - n] & int(column[q]))
        best = c if best is None else min(best, c)
    return best


def path_changes(parent, child, entries, n, i, j, site):
    """the changes at `site` on the edges of the path between leaves i and j"""
    up = {int(c): (int(p), e) for e, (p, c) in enumerate(zip(parent, child))}

    def chain(v):
        edges = []
        while v in up:
            v, e = up[v]
            edges.append(e)
        return edges
    if n == 2:
        path = {0}
    else:
        a, b = chain(i), chain(j)
        path = set(a) ^ set(b)
    changed = {e for s, e, _ in entries if s == site}
    return len(path & changed)


# ---- trees as edge arrays ------------------------------------------------------------------------------------------------------------
def tree_from_joins(n, joins, last):
    """joins: [(a, b)] for t = 0 .. n - 4 (node n + t); last: the three remaining nodes -> parent, child (uint32) as tracs_nj_edges"""
    parent, child = [], []
    for t, (a, b) in enumerate(joins):
        a, b = sorted((a, b))
        parent += [n + t, n + t]
        child += [a, b]
    if n >= 3:
        parent += [2 * n - 3] * 3
        child += sorted(last)
    elif n == 2:
        parent, child = [0], [1]
    return np.array(parent, np.uint32), np.array(child, np.uint32)


def random_tree(n, rng):
    """a random join order"""
    live = list(range(n))
    joins = []
    for t in range(max(n - 3, 0)):
        i, j = rng.choice(len(live), 2, replace=False)
        a, b = live[i], live[j]
        live = [v for v in live if v not in (a, b)] + [n + t]
        joins.append((a, b))
    return tree_from_joins(n, joins, live)


def caterpillar(n):
    """((0, 1), 2), 3), ...: n deep"""
    joins, cur = [], 0
    for t in range(max(n - 3, 0)):
        joins.append((cur, t + 1))
        cur = n + t
    last = [cur] + list(range(max(n - 3, 0) + 1, n)) if n >= 3 else []
    return tree_from_joins(n, joins, last)


def balanced(n):
    """pairs of the oldest two live nodes, level by level"""
    live = list(range(n))
    joins = []
    for t in range(max(n - 3, 0)):
        a, b = live[0], live[1]
        live = live[2:] + [n + t]
        joins.append((a, b))
    return tree_from_joins(n, joins, live)


LETTERS = "XACMGRSVTWYHKDBN"          # mask -> IUPAC letter


def masks_to_fasta(masks):
    return ["".join(LETTERS[int(m)] for m in row) for row in np.asarray(masks)]
