"""Transfer bootstrap support as DESIGN.md 3.19 defines it, restated for the tests by brute force over Python integers as bitmasks: the
leaves below every edge, h, delta, phi, the lighter side p, the sums and the support x; beside it a restatement of the program builder
(tracs_tree_transfer_program) and an interpreter of a program, which is what one lane of transfer_phi_kernel does."""
import numpy as np

NONE = 0xFFFFFFFF
NONE64 = 0xFFFFFFFFFFFFFFFF
INTERNAL = 0x80000000


_pop = int.bit_count if hasattr(int, "bit_count") else (lambda x: bin(x).count("1"))


def below(n, parent, child):
    """per edge, the leaves below its child as a bitmask (edges in creation order: a child is complete before it is hung)"""
    under, out = {}, []
    for p, c in zip(np.asarray(parent).tolist(), np.asarray(child).tolist()):
        m = (1 << c) if c < n else under[c]
        under[p] = under.get(p, 0) | m
        out.append(m)
    return out


def phi(n, main, rep):
    """per edge of `main`: for an internal edge the smallest delta over ALL edges of `rep`, else NONE"""
    S = below(n, main[0], main[1])
    T = [(m, _pop(m)) for m in below(n, rep[0], rep[1])]
    out = []
    for c, s_mask in zip(np.asarray(main[1]).tolist(), S):
        if c < n or n < 4:
            out.append(NONE)
            continue
        s = _pop(s_mask)
        best = None
        for t_mask, t in T:
            h = s + t - 2 * _pop(s_mask & t_mask)
            d = min(h, n - h)
            best = d if best is None or d < best else best
        out.append(best)
    return out


def light(n, main):
    """per edge of `main`: p = min(|S|, n - |S|) for an internal edge, else NONE"""
    return [NONE if (c < n or n < 4) else min(_pop(m), n - _pop(m))
            for c, m in zip(np.asarray(main[1]).tolist(), below(n, main[0], main[1]))]


def transfer(n, main, reps):
    """-> (sum_phi, p, x) per edge of `main`: the integer sum of phi over the replicates, the lighter side, and the double
    1.0 - float(sum) / float(B (p - 1)); NONE64, NONE and NaN on leaf edges"""
    p = light(n, main)
    per_rep = [phi(n, main, rep) for rep in reps]
    B = len(reps)
    sums, xs = [], []
    for e, pe in enumerate(p):
        if pe == NONE:
            sums.append(NONE64)
            xs.append(float("nan"))
            continue
        assert pe >= 2
        S = sum(r[e] for r in per_rep)
        D = B * (pe - 1)
        assert 0 <= S <= D
        sums.append(S)
        xs.append(1.0 - float(S) / float(D))
    return sums, p, xs


def program(n, parent, child):
    """the post-order program of a tree: a leaf l is the entry l, a joined node v the entry INTERNAL | |T_v| after its two subtrees, the
    top node nothing; children largest subtree first (ties: lower id).  -> (entries, the deepest the stack gets)"""
    parent, child = np.asarray(parent).tolist(), np.asarray(child).tolist()
    size, kids = {}, {}
    for p, c in zip(parent, child):
        size[p] = size.get(p, 0) + (1 if c < n else size[c])
        kids.setdefault(p, []).append(c)
    top = parent[-1]
    order = lambda v: sorted(kids[v], key=lambda c: (-(1 if c < n else size[c]), c))      # noqa: E731
    out, sp, deepest = [], 0, 0
    stack = [(top, iter(order(top)))]
    while stack:
        node, it = stack[-1]
        c = next(it, None)
        if c is None:
            stack.pop()
            if node != top:
                out.append(INTERNAL | size[node])
                sp -= 1
        elif c < n:
            out.append(c)
            sp += 1
            deepest = max(deepest, sp)
        else:
            stack.append((c, iter(order(c))))
    return out, deepest


def run_program(n, entries, s_mask):
    """phi of the set s_mask against the tree behind `entries`: leaf -- push [leaf in S]; joined node -- pop two, push the sum; every
    entry gives h = s + t - 2 c and delta = min(h, n - h).  -> (phi, the deepest the stack got)"""
    s = _pop(s_mask)
    stack, best, deepest = [], None, 0
    for e in entries:
        if e & INTERNAL:
            t = e & ~INTERNAL
            b, a = stack.pop(), stack.pop()
            stack.append(a + b)
        else:
            t = 1
            stack.append((s_mask >> e) & 1)
        deepest = max(deepest, len(stack))
        h = s + t - 2 * stack[-1]
        d = min(h, n - h)
        best = d if best is None or d < best else best
    assert len(stack) == 3 and sum(stack) == s
    return best, deepest


def balanced_edges(n):
    """parent, child of the tree that joins the two oldest active nodes until three are left (n a power of two: leaves pair up, then
    the pairs, ... -- perfectly balanced below the top node's three children)"""
    active, P, Ch = list(range(n)), [], []
    for t in range(n - 3):
        a, b = active[0], active[1]
        P += [n + t, n + t]
        Ch += sorted([a, b])
        active = active[2:] + [n + t]
    P += [2 * n - 3] * 3
    Ch += sorted(active)
    return np.array(P, np.uint32), np.array(Ch, np.uint32)


def edges_of_adjacency(n, adj, root):
    """an unrooted binary tree (node -> set of neighbours; leaves 0 .. n - 1, every other node of degree three) as parent, child in
    creation order: hung from `root`, the other inner nodes numbered n, n + 1, ... as an iterative post-order completes them"""
    label = {v: v for v in range(n)}
    P, Ch = [], []
    stack = [(root, None, iter(sorted(adj[root])))]
    while stack:
        v, up, it = stack[-1]
        w = next(it, None)
        if w is None:
            stack.pop()
            label[v] = n + len(P) // 2 if v != root else 2 * n - 3
            kids = sorted(label[k] for k in adj[v] if k != up)
            P += [label[v]] * len(kids)
            Ch += kids
        elif w != up and w >= n:
            stack.append((w, v, iter(sorted(adj[w]))))
    assert len(P) == 2 * n - 3
    return np.array(P, np.uint32), np.array(Ch, np.uint32)


def rehung(n, parent, child, leaf, where):
    """the tree with `leaf` taken out and hung on the `where`-th edge of what is left -> parent, child in creation order"""
    adj = {}
    for p, c in zip(np.asarray(parent).tolist(), np.asarray(child).tolist()):
        adj.setdefault(p, set()).add(c)
        adj.setdefault(c, set()).add(p)
    (q,) = adj[leaf]
    a, b = sorted(adj[q] - {leaf})                                           # q is dissolved: its other two neighbours are joined
    adj[a].discard(q); adj[b].discard(q); adj[a].add(b); adj[b].add(a)
    edges = sorted({(min(u, v), max(u, v)) for u in adj if u not in (q, leaf) for v in adj[u]})
    u, v = edges[where % len(edges)]
    adj[u].discard(v); adj[v].discard(u); adj[u].add(q); adj[v].add(q)
    adj[q] = {u, v, leaf}
    return edges_of_adjacency(n, adj, q)
