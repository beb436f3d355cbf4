"""BIONJ (Gascuel 1997) as DESIGN.md 3.23 defines it, restated for the tests: in numpy float64 with the definition's operation order
(bionj_records; the edges are nj_ref.nj_edges of the records, unchanged) and in exact rational arithmetic (bionj_exact).

What BIONJ shares with neighbour joining (tests/nj_ref.py): IEEE float64, one rounding per operation, no fma; Q and
the tie rule (Q, lower id, higher id); the record (a, b, D_ab, R_a, R_b) with r = n - t; the three-node end; n <= 3.

What is new, with r > 3 active nodes and the join (a, b), a < b BY NODE ID.  Every pair of brackets is one rounding:
    V = D and RV = R at the start, bit for bit
    l_a    = (0.5 * D_ab) + ((R_a - R_b) / (2.0 * (r - 2)))        the host's formula for the lengths, the same operations
    l_b    = D_ab - l_a
    lambda = 0.5                                                    if V_ab == 0
             0.5 + ((RV_b - RV_a) / ((2.0 * (r - 2)) * V_ab))       else; then 0 if it is < 0, 1 if it is > 1
    mu     = 1.0 - lambda
    lmv    = (lambda * mu) * V_ab
    D_uk   = (lambda * (D_ak - l_a)) + (mu * (D_bk - l_b))
    V_uk   = ((lambda * V_ak) + (mu * V_bk)) - lmv
    R_k   <- (R_k - (D_ak + D_bk)) + D_uk
    RV_k  <- (RV_k - (V_ak + V_bk)) + V_uk
    R_u    = (lambda * ((R_a - D_ab) - ((r - 2) * l_a))) + (mu * ((R_b - D_ab) - ((r - 2) * l_b)))
    RV_u   = ((lambda * (RV_a - V_ab)) + (mu * (RV_b - V_ab))) - ((r - 2) * lmv)
RV_b - RV_a is Gascuel's sum over k != a, b of V_bk - V_ak written through the running row sums: V is symmetric with a zero diagonal,
so the cells (a, a), (a, b), (b, a), (b, b) cancel.  There is no order-dependent reduction and nothing beyond neighbour joining's
three steps.  mu is rounded, so the formulas are not bitwise symmetric in a and b: a is the lower id, whatever slot it lives in.
Nothing else is clamped: D, V and the lengths may go negative on data that is not tree-like.

Nodes as in nj_ref: the active nodes are kept in id order, so the first minimum of Q over the upper triangle in row-major order is
the smallest (Q, lower id, higher id), and i < j there means a < b."""
from fractions import Fraction

import numpy as np

import nj_ref

NONE = nj_ref.NONE


def bionj_records(D, trace=None):
    """-> what nj_ref.nj_records returns, for BIONJ.  trace (a list): per join (lambda, V_ab, lambda before the clamp) is appended."""
    D = np.array(D, np.float64)
    n = D.shape[0]
    if n <= 3:
        return nj_ref.nj_records(D)
    a, b, dab, ra, rb = [], [], [], [], []
    ids = list(range(n))
    R = nj_ref.row_sums(D)
    V, RV = D.copy(), R.copy()
    t = 0
    half, one, zero, two = np.float64(0.5), np.float64(1.0), np.float64(0.0), np.float64(2.0)
    with np.errstate(all="ignore"):
        while len(ids) > 3:
            r = len(ids)
            rm2 = np.float64(r - 2)
            Q = (rm2 * D) - (R[:, None] + R[None, :])
            Q[np.tril_indices(r)] = np.inf
            Q[np.isnan(Q)] = np.inf
            i, j = divmod(int(np.argmin(Q)), r)
            d, v = D[i, j], V[i, j]
            a.append(ids[i]); b.append(ids[j]); dab.append(d); ra.append(R[i]); rb.append(R[j])
            den = two * rm2
            la = (half * d) + ((R[i] - R[j]) / den)
            lb = d - la
            lam = raw = half
            if v != zero:
                lam = raw = half + ((RV[j] - RV[i]) / (den * v))
                if lam < zero:
                    lam = zero
                if lam > one:
                    lam = one
            mu = one - lam
            lmv = (lam * mu) * v
            if trace is not None:
                trace.append((float(lam), float(v), float(raw)))
            du = (lam * (D[i] - la)) + (mu * (D[j] - lb))
            vu = ((lam * V[i]) + (mu * V[j])) - lmv
            Rn = (R - (D[i] + D[j])) + du
            RVn = (RV - (V[i] + V[j])) + vu
            Ru = (lam * ((R[i] - d) - (rm2 * la))) + (mu * ((R[j] - d) - (rm2 * lb)))
            RVu = ((lam * (RV[i] - v)) + (mu * (RV[j] - v))) - (rm2 * lmv)
            keep = [k for k in range(r) if k != i and k != j]

            def reduced(M, row):
                Mn = np.zeros((r - 1, r - 1), np.float64)
                Mn[:r - 2, :r - 2] = M[np.ix_(keep, keep)]
                Mn[r - 2, :r - 2] = row[keep]
                Mn[:r - 2, r - 2] = row[keep]
                return Mn
            D, V = reduced(D, du), reduced(V, vu)
            R = np.concatenate([Rn[keep], [Ru]])
            RV = np.concatenate([RVn[keep], [RVu]])
            ids = [ids[k] for k in keep] + [n + t]
            t += 1
    last_ids, last_d = np.zeros(3, np.uint32), np.zeros(3, np.float64)
    last_ids[:] = ids
    last_d[:] = (D[0, 1], D[0, 2], D[1, 2])
    return nj_ref._rec(a, b, dab, ra, rb), last_ids, last_d


def bionj(D):
    """the reference's edges for a matrix: the lengths are neighbour joining's formula on BIONJ's records"""
    D = np.asarray(D, np.float64)
    rec, ids, d = bionj_records(D)
    return nj_ref.nj_edges(D.shape[0], rec, ids, d)


def bionj_exact(D, check=None):
    """The same algorithm and tie rule in fractions.Fraction on an integer matrix (n >= 4) -> [(a, b, D_ab)] per join, [(parent,
    child, length)] for all 2n - 3 edges, and ties: per join whether two pairs shared the smallest Q exactly, as (r, tied).
    check(r, lam, gascuel_lam, R, RV, M, W): called per join with lambda from the running sums, lambda from Gascuel's explicit sum
    over k != a, b (both clamped), and the running sums beside the matrices they must be the row sums of."""
    n = len(D)
    M = [[Fraction(int(D[i][j])) for j in range(n)] for i in range(n)]
    W = [row[:] for row in M]
    ids = list(range(n))
    R = [sum(M[m][k] for m in range(n)) for k in range(n)]
    RV = R[:]
    joins, edges, ties = [], [], []
    clamp = lambda x: min(max(x, Fraction(0)), Fraction(1))           # noqa: E731
    t = 0
    while len(ids) > 3:
        r = len(ids)
        best, tied = None, False
        for i in range(r):
            for j in range(i + 1, r):
                q = (r - 2) * M[i][j] - (R[i] + R[j])
                if best is None or q < best[0]:
                    best, tied = (q, i, j), False
                elif q == best[0]:
                    tied = True
        ties.append((r, tied))
        _, i, j = best
        d, v = M[i][j], W[i][j]
        joins.append((ids[i], ids[j], d))
        la = d / 2 + (R[i] - R[j]) / (2 * (r - 2))
        lb = d - la
        edges += [(n + t, ids[i], la), (n + t, ids[j], lb)]
        keep = [k for k in range(r) if k != i and k != j]
        lam = Fraction(1, 2) if v == 0 else clamp(Fraction(1, 2) + (RV[j] - RV[i]) / (2 * (r - 2) * v))
        if check is not None:
            explicit = Fraction(1, 2) if v == 0 else clamp(Fraction(1, 2) + sum(W[j][k] - W[i][k] for k in keep) / (2 * (r - 2) * v))
            check(r, lam, explicit, R, RV, M, W)
        mu = 1 - lam
        du = [lam * (M[i][k] - la) + mu * (M[j][k] - lb) for k in range(r)]
        vu = [lam * W[i][k] + mu * W[j][k] - lam * mu * v for k in range(r)]
        Rn = [R[k] - (M[i][k] + M[j][k]) + du[k] for k in range(r)]
        RVn = [RV[k] - (W[i][k] + W[j][k]) + vu[k] for k in range(r)]
        Ru = lam * ((R[i] - d) - (r - 2) * la) + mu * ((R[j] - d) - (r - 2) * lb)
        RVu = lam * (RV[i] - v) + mu * (RV[j] - v) - (r - 2) * lam * mu * v
        M = [[M[p][q] for q in keep] + [du[p]] for p in keep] + [[du[q] for q in keep] + [Fraction(0)]]
        W = [[W[p][q] for q in keep] + [vu[p]] for p in keep] + [[vu[q] for q in keep] + [Fraction(0)]]
        R = [Rn[k] for k in keep] + [Ru]
        RV = [RVn[k] for k in keep] + [RVu]
        ids = [ids[k] for k in keep] + [n + t]
        t += 1
    if check is not None:
        check(3, None, None, R, RV, M, W)
    dxy, dxz, dyz = M[0][1], M[0][2], M[1][2]
    top = 2 * n - 3
    edges += [(top, ids[0], (dxy + dxz - dyz) / 2), (top, ids[1], (dxy + dyz - dxz) / 2), (top, ids[2], (dxz + dyz - dxy) / 2)]
    return joins, edges, ties


def exact_splits(n, edges):
    """the split set (nj_ref.splits_of's keys) of bionj_exact's edges"""
    parent = np.array([e[0] for e in edges], np.uint32)
    child = np.array([e[1] for e in edges], np.uint32)
    return set(nj_ref.splits_of(n, parent, child, np.zeros(len(edges))))


# the 6 x 6 matrix on which neighbour joining and BIONJ give different trees (tests/test_bionj_ref.py confirms it on both references)
NJ_DIFFERS = np.array([[0, 43, 59, 82, 12, 46],
                       [43, 0, 60, 81, 46, 27],
                       [59, 60, 0, 18, 73, 52],
                       [82, 81, 18, 0, 82, 48],
                       [12, 46, 73, 82, 0, 37],
                       [46, 27, 52, 48, 37, 0]], np.float64)


def noisy_tree_metric(n, seed, noise=2, max_len=9):
    """an integer tree metric with symmetric integer noise in [-noise, noise] on every cell, kept >= 0 off the diagonal"""
    rng = np.random.default_rng(seed)
    D = nj_ref.random_tree_metric(n, rng, max_len)[0]
    E = np.triu(rng.integers(-noise, noise + 1, (n, n)), 1)
    D = np.maximum(D + E + E.T, 0.0)
    np.fill_diagonal(D, 0.0)
    return D
