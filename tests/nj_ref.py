"""Neighbour joining as DESIGN.md 3.17 defines it, restated for the tests: in numpy float64 with the definition's operation order
(nj_records, nj_edges), in exact rational arithmetic (nj_exact), plus what the tree tests share: a random integer tree metric, split
extraction and a Newick parser.

Nodes: leaves 0 .. n - 1, join number t makes n + t.  The active nodes are kept in id order, so the first minimum of Q over the upper
triangle in row-major order IS the smallest (Q, lower id, higher id): the new node has the largest id and is appended."""
from fractions import Fraction

import numpy as np

NONE = 0xFFFFFFFF


def row_sums(D):
    """R_k = the sum of D_mk over m = 0 .. n - 1 in that order, one add at a time"""
    R = np.zeros(D.shape[0], np.float64)
    for m in range(D.shape[0]):
        R = R + D[m]
    return R


def nj_records(D):
    """-> a, b (uint32), d_ab, r_a, r_b (float64), each n - 3 long; last_ids (uint32[3]), last_d (float64[3]: D_xy, D_xz, D_yz).
    n = 2: last_ids = (0, 1, NONE), last_d[0] = D_01.  n < 2: no ids."""
    D = np.array(D, np.float64)
    n = D.shape[0]
    a, b, dab, ra, rb = [], [], [], [], []
    last_ids, last_d = np.full(3, NONE, np.uint32), np.zeros(3, np.float64)
    if n < 2:
        return _rec(a, b, dab, ra, rb), last_ids, last_d
    if n == 2:
        last_ids[:2] = (0, 1)
        last_d[0] = D[0, 1]
        return _rec(a, b, dab, ra, rb), last_ids, last_d
    ids = list(range(n))
    R = row_sums(D)
    t = 0
    while len(ids) > 3:
        r = len(ids)
        Q = (float(r - 2) * D) - (R[:, None] + R[None, :])
        Q[np.tril_indices(r)] = np.inf
        Q[np.isnan(Q)] = np.inf
        i, j = divmod(int(np.argmin(Q)), r)              # the first minimum in row-major order: the smallest (Q, id_i, id_j)
        d = D[i, j]
        a.append(ids[i]); b.append(ids[j]); dab.append(d); ra.append(R[i]); rb.append(R[j])
        s = D[i] + D[j]
        du = (s - d) * 0.5
        Rn = (R - s) + du
        Ru = ((R[i] + R[j]) - (float(r) * d)) * 0.5
        keep = [k for k in range(r) if k != i and k != j]
        Dn = np.zeros((r - 1, r - 1), np.float64)
        Dn[:r - 2, :r - 2] = D[np.ix_(keep, keep)]
        Dn[r - 2, :r - 2] = du[keep]
        Dn[:r - 2, r - 2] = du[keep]
        D = Dn
        R = np.concatenate([Rn[keep], [Ru]])
        ids = [ids[k] for k in keep] + [n + t]
        t += 1
    last_ids[:] = ids
    last_d[:] = (D[0, 1], D[0, 2], D[1, 2])
    return _rec(a, b, dab, ra, rb), last_ids, last_d


def _rec(a, b, dab, ra, rb):
    return (np.array(a, np.uint32), np.array(b, np.uint32), np.array(dab, np.float64), np.array(ra, np.float64), np.array(rb, np.float64))


def nj_edges(n, rec, last_ids, last_d):
    """parent, child (uint32), length (float64): the 2n - 3 edges in creation order, lengths with the definition's roundings.
    n = 2: the one edge (0, 1, D_01); n < 2: none."""
    a, b, dab, ra, rb = rec
    P, Ch, Ln = [], [], []
    if n == 2:
        P, Ch, Ln = [0], [1], [last_d[0]]
    elif n >= 3:
        for t in range(n - 3):
            r = float(n - t)
            la = (0.5 * dab[t]) + ((ra[t] - rb[t]) / (2.0 * (r - 2.0)))
            lb = dab[t] - la
            P += [n + t, n + t]; Ch += [a[t], b[t]]; Ln += [la, lb]
        dxy, dxz, dyz = (np.float64(v) for v in last_d)
        top = 2 * n - 3
        P += [top] * 3
        Ch += [int(v) for v in last_ids]
        Ln += [((dxy + dxz) - dyz) * 0.5, ((dxy + dyz) - dxz) * 0.5, ((dxz + dyz) - dxy) * 0.5]
    return np.array(P, np.uint32), np.array(Ch, np.uint32), np.array(Ln, np.float64)


def nj(D):
    """the reference's edges for a matrix"""
    D = np.asarray(D, np.float64)
    rec, ids, d = nj_records(D)
    return nj_edges(D.shape[0], rec, ids, d)


def nj_exact(D):
    """The same algorithm and tie rule in fractions.Fraction on an integer matrix -> [(a, b, D_ab)] per join, [(parent, child,
    length)] for all 2n - 3 edges (n >= 3)."""
    n = len(D)
    M = [[Fraction(int(D[i][j])) for j in range(n)] for i in range(n)]
    ids = list(range(n))
    R = [sum(M[m][k] for m in range(n)) for k in range(n)]
    joins, edges = [], []
    t = 0
    while len(ids) > 3:
        r = len(ids)
        best = None
        for i in range(r):
            for j in range(i + 1, r):
                q = (r - 2) * M[i][j] - (R[i] + R[j])
                if best is None or q < best[0]:
                    best = (q, i, j)
        _, i, j = best
        d = M[i][j]
        joins.append((ids[i], ids[j], d))
        la = d / 2 + (R[i] - R[j]) / (2 * (r - 2))
        edges += [(n + t, ids[i], la), (n + t, ids[j], d - la)]
        keep = [k for k in range(r) if k != i and k != j]
        du = [(M[i][k] + M[j][k] - d) / 2 for k in range(r)]
        Rn = [R[k] - (M[i][k] + M[j][k]) + du[k] for k in range(r)]
        Ru = (R[i] + R[j] - r * d) / 2
        M = [[M[p][q] for q in keep] + [du[p]] for p in keep] + [[du[q] for q in keep] + [Fraction(0)]]
        R = [Rn[k] for k in keep] + [Ru]
        ids = [ids[k] for k in keep] + [n + t]
        t += 1
    dxy, dxz, dyz = M[0][1], M[0][2], M[1][2]
    top = 2 * n - 3
    edges += [(top, ids[0], (dxy + dxz - dyz) / 2), (top, ids[1], (dxy + dyz - dxz) / 2), (top, ids[2], (dxz + dyz - dxy) / 2)]
    return joins, edges


def random_tree_metric(n, rng, max_len=9):
    """An unrooted binary tree over n >= 3 leaves with integer branch lengths in [1, max_len] (leaves are inserted one by one into a
    random edge) -> D (float64, integer-valued path lengths), {split: length} as splits_of gives them."""
    edges = [[n, 0], [n, 1], [n, 2]]                      # (inner node, other end)
    nxt = n + 1
    for leaf in range(3, n):
        e = int(rng.integers(len(edges)))
        u, v = edges[e]
        edges[e] = [u, nxt]
        edges += [[nxt, v], [nxt, leaf]]
        nxt += 1
    w = [int(x) for x in rng.integers(1, max_len + 1, len(edges))]
    nodes = nxt
    adj = [[] for _ in range(nodes)]
    for (u, v), x in zip(edges, w):
        adj[u].append((v, x)); adj[v].append((u, x))
    D = np.zeros((n, n), np.float64)
    for s in range(n):
        dist = [-1] * nodes
        dist[s] = 0
        stack = [s]
        while stack:
            u = stack.pop()
            for v, x in adj[u]:
                if dist[v] < 0:
                    dist[v] = dist[u] + x
                    stack.append(v)
        D[s] = dist[:n]
    # splits: root at leaf 0, the leaves below every other node
    order, par = [], {0: (None, 0)}
    stack = [0]
    while stack:
        u = stack.pop()
        order.append(u)
        for v, x in adj[u]:
            if v not in par:
                par[v] = (u, x)
                stack.append(v)
    below = [0] * nodes
    splits = {}
    for u in reversed(order):
        if u < n:
            below[u] |= 1 << u
        p, x = par[u]
        if p is not None:
            below[p] |= below[u]
            splits[_norm(below[u], n)] = float(x)
    return D, splits


def _norm(mask, n):
    """a split as the bitmask of the side without leaf 0"""
    return mask if not (mask & 1) else ((1 << n) - 1) & ~mask


def splits_of(n, parent, child, length):
    """{split: length} of a tree given as edges in creation order (children before their parents; leaves are [0, n))"""
    below = {}
    out = {}
    for p, c, x in zip(parent.tolist(), child.tolist(), length.tolist()):
        m = (1 << c) if c < n else below[c]
        below[p] = below.get(p, 0) | m
        out[_norm(m, n)] = x
    return out


def parse_newick(text):
    """One Newick tree -> nodes [(parent index or None, label or None, length or None)] in the order they open (the root first).
    No recursion.  Quoted labels are unquoted ('' -> ')."""
    s = text.strip()
    assert s.endswith(";"), "no terminating ;"
    s = s[:-1]
    nodes = [[None, None, None]]
    cur = 0
    i = 0

    def label_and_length(i, node):
        if i < len(s) and s[i] == "'":
            j, buf = i + 1, []
            while True:
                assert j < len(s), "unterminated quote"
                if s[j] == "'":
                    if j + 1 < len(s) and s[j + 1] == "'":
                        buf.append("'"); j += 2
                        continue
                    break
                buf.append(s[j]); j += 1
            nodes[node][1] = "".join(buf)
            i = j + 1
        else:
            j = i
            while j < len(s) and s[j] not in ":,();":
                j += 1
            if j > i:
                nodes[node][1] = s[i:j]
            i = j
        if i < len(s) and s[i] == ":":
            j = i + 1
            while j < len(s) and s[j] not in ",()":
                j += 1
            nodes[node][2] = float(s[i + 1:j])
            i = j
        return i

    if not s.startswith("("):
        label_and_length(0, 0)
        return [tuple(x) for x in nodes]
    depth = 0
    while i < len(s):
        ch = s[i]
        if ch == "(":
            if depth:
                nodes.append([cur, None, None])
                cur = len(nodes) - 1
            depth += 1
            i += 1
            if s[i] not in "(":
                nodes.append([cur, None, None])
                i = label_and_length(i, len(nodes) - 1)
        elif ch == ",":
            i += 1
            if s[i] != "(":
                nodes.append([cur, None, None])
                i = label_and_length(i, len(nodes) - 1)
        elif ch == ")":
            depth -= 1
            i = label_and_length(i + 1, cur)
            cur = nodes[cur][0] if nodes[cur][0] is not None else 0
        else:
            raise AssertionError("unexpected %r at %d" % (ch, i))
    assert depth == 0, "unbalanced parentheses"
    return [tuple(x) for x in nodes]


def newick_splits(nodes, names):
    """{split: length} of a parsed tree whose leaves carry `names` (index = leaf id); also checks the leaves are exactly the names"""
    n = len(names)
    index = {nm: k for k, nm in enumerate(names)}
    assert len(index) == n
    has_child = [False] * len(nodes)
    for p, _, _ in nodes:
        if p is not None:
            has_child[p] = True
    leaves = [lab for k, (p, lab, ln) in enumerate(nodes) if not has_child[k]]
    assert sorted(leaves) == sorted(names), "the tree's leaves are not the samples"
    below = [0] * len(nodes)
    out = {}
    for k in range(len(nodes) - 1, -1, -1):               # children open after their parents
        p, lab, ln = nodes[k]
        if not has_child[k]:
            below[k] = 1 << index[lab]
        if p is not None:
            below[p] |= below[k]
            out[_norm(below[k], n)] = ln
    return out
