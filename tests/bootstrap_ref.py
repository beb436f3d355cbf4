"""Bootstrap replicates as DESIGN.md 3.18 defines them, restated for the tests in numpy and Python integers: the draws (the 128-bit
product as a Python integer), the weights, the repeated text, brute-force SNP distances, the replicate tree (nj_ref.nj), splits and
supports."""
import numpy as np

import nj_ref

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
NONE = 0xFFFFFFFF


def mix(x):
    z = x & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, b):
    return mix((seed + GOLDEN * (b + 1)) & M64)


def u(seed, b, t):
    return mix((key(seed, b) + GOLDEN * (t + 1)) & M64)


def draw(seed, b, t, L):
    """c(b, t): the high half of the 128-bit product u L"""
    return (u(seed, b, t) * L) >> 64


def weights(L, seed, b):
    """w_b: int64[L], how often each column is drawn"""
    k = key(seed, b)
    w = np.zeros(L, np.int64)
    for t in range(L):
        w[(mix((k + GOLDEN * (t + 1)) & M64) * L) >> 64] += 1
    return w


def repeated(seqs, w):
    """column c repeated w[c] times, columns in ascending c, every sample"""
    return np.ascontiguousarray(np.repeat(seqs, np.asarray(w, np.int64), axis=1))


# allele masks as the pack stores them (IUPAC letters set several bits, anything else all four), upper and lower case
_BITS = {"A": 1, "C": 2, "G": 4, "T": 8, "M": 3, "R": 5, "S": 6, "V": 7, "W": 9, "Y": 10, "H": 11, "K": 12, "D": 13, "B": 14}
MASKS = np.full(256, 15, np.uint8)
for _ch, _m in _BITS.items():
    MASKS[ord(_ch)] = _m
    MASKS[ord(_ch.lower())] = _m
CANONICAL = np.frombuffer(b"XACMGRSVTWYHKDBN", np.uint8)


def canonical(seqs):
    """the text tracs_alignment_unpack gives: "XACMGRSVTWYHKDBN"[mask]"""
    return CANONICAL[MASKS[seqs]]


def snp_matrix(seqs, w=None):
    """d(i, j) = the sum of w(c) over the columns at which the two masks are disjoint (w None: 1 each), brute force -> int64[n, n]"""
    m = MASKS[seqs]
    n, L = m.shape
    w = np.ones(L, np.int64) if w is None else np.asarray(w, np.int64)
    D = np.zeros((n, n), np.int64)
    for i in range(n):
        D[i] = (((m[i][None, :] & m) == 0) * w[None, :]).sum(axis=1)
    return D


def differs(seqs):
    """bool[L]: two samples have disjoint masks there"""
    m = MASKS[seqs]
    out = np.zeros(m.shape[1], bool)
    for i in range(m.shape[0]):
        out |= ((m[i][None, :] & m) == 0).any(axis=0)
    return out


def replicate_tree(seqs, seed, b):
    """the edges of replicate b: neighbour joining on the distances of the repeated text"""
    return nj_ref.nj(snp_matrix(seqs, weights(seqs.shape[1], seed, b)).astype(np.float64))


def internal_splits(n, parent, child):
    """{split of each internal edge: its index}: the leaves below the child as a bitmask, on the side without leaf 0"""
    below, out = {}, {}
    for e, (p, c) in enumerate(zip(np.asarray(parent).tolist(), np.asarray(child).tolist())):
        m = (1 << c) if c < n else below[c]
        below[p] = below.get(p, 0) | m
        if c >= n:
            out[nj_ref._norm(m, n)] = e
    return out


def supports(n, main, replicates):
    """uint32 per edge of `main` = (parent, child[, length]): for an internal edge the number of replicate trees that have its split,
    else NONE"""
    parent, child = main[0], main[1]
    out = np.full(len(parent), NONE, np.uint32)
    if n < 4:
        return out
    mine = internal_splits(n, parent, child)
    assert len(mine) == n - 3
    for e in mine.values():
        out[e] = 0
    for rep in replicates:
        theirs = internal_splits(n, rep[0], rep[1])
        for split, e in mine.items():
            if split in theirs:
                out[e] += 1
    return out


def random_tree_edges(n, rng):
    """parent, child (uint32) of a random binary tree over n >= 3 leaves in creation order: join two random active nodes until three
    are left"""
    active = list(range(n))
    P, Ch = [], []
    for t in range(n - 3):
        i, j = sorted(rng.choice(len(active), 2, replace=False).tolist())
        a, b = active[i], active[j]
        P += [n + t, n + t]
        Ch += [a, b]
        active = [x for k, x in enumerate(active) if k not in (i, j)] + [n + t]
    P += [2 * n - 3] * 3
    Ch += sorted(active)
    return np.array(P, np.uint32), np.array(Ch, np.uint32)


def caterpillar_edges(order):
    """parent, child of the caterpillar that joins the leaves in `order` one after the other (n deep)"""
    n = len(order)
    P, Ch = [n, n], sorted(order[:2])
    for t in range(1, n - 3):
        P += [n + t, n + t]
        Ch += [order[t + 1], n + t - 1]
    P += [2 * n - 3] * 3
    Ch += sorted([order[n - 2], order[n - 1]]) + [2 * n - 4]
    return np.array(P, np.uint32), np.array(Ch, np.uint32)


def outbreak_alignment():
    """The end-to-end fixture: 24 samples x 600 columns -- a clade (samples 0 .. 7) that 40 columns separate from the rest, a clade
    (8 .. 11) that a single column separates, a pair of identical samples (22, 23), a few private changes per sample, N and partial
    codes -> uint8[24, 600]"""
    rng = np.random.default_rng(20)
    n, L = 24, 600
    bases = np.frombuffer(b"ACGT", np.uint8)
    anc = rng.integers(0, 4, L)
    idx = np.tile(anc, (n, 1))
    cols = rng.permutation(L)
    idx[0:8, cols[:40]] = (idx[0:8, cols[:40]] + 1) % 4                     # 40 columns
    idx[8:12, cols[40]] = (idx[8:12, cols[40]] + 2) % 4                     # one column
    idx[12:18, cols[41:44]] = (idx[12:18, cols[41:44]] + 3) % 4             # a clade on three columns
    at = 44
    for s in range(n - 1):                                                  # private changes, none in the last sample
        k = int(rng.integers(1, 4))
        idx[s, cols[at:at + k]] = (idx[s, cols[at:at + k]] + 1) % 4
        at += k
    idx[2:4, cols[at:at + 2]] = (idx[2:4, cols[at:at + 2]] + 2) % 4         # structure inside the big clade
    idx[4:8, cols[at + 2:at + 3]] = (idx[4:8, cols[at + 2:at + 3]] + 2) % 4
    idx[22] = idx[23]
    seqs = bases[idx]
    seqs[rng.random((n, L)) < 0.01] = ord("N")
    seqs[rng.random((n, L)) < 0.003] = ord("R")
    seqs[rng.random((n, L)) < 0.003] = ord("y")
    seqs[22] = seqs[23]
    return np.ascontiguousarray(seqs)
