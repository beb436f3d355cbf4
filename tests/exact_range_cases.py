"""Inputs, lengths and the plain int64 reference shared by tests/test_fp32_range_model.py (CPU) and tests/test_gpu_exact_range.py (GPU).

The three matrix-core forms of the pair kernel (csrc/pairsnp_mfma.hip) keep their sums in fp32 accumulators, exact only while no
partial sum of a workgroup's site range reaches 2^24; the host bounds the ranges (csrc/pairsnp.hip: choose_route's max_gps applied by
pairs_one_launch, thr_prefix_groups and thr_remainder_split; count_pass's own 2^16 groups).  The cases here are the smallest inputs
that tell a right bound from a wrong one: a few samples, alignments longer than one exact range, and one named pair per case whose
sum over the whole alignment exceeds 2^24 -- asserted from the reference (assert_precondition), never assumed.

Everything is deterministic: np.random.default_rng with the seeds below."""
import numpy as np

SITES_PER_GROUP = 128                     # csrc/common.h

L_PAIR = 3 * (1 << 21) + 77               # consensus, general: beyond both bounds (2^22, 2^21 sites); the last group is clipped
L_COUNT = (1 << 24) + (1 << 21) + 77      # count: NN(1, 2) ~ 0.95 L ~ 17.9 M > 2^24

BOUND_SITES = {"consensus": 1 << 22, "general": 1 << 21, "count": 1 << 23}      # sites per range at most, as the host code has them
STAGE_GROUPS = {"consensus": 1, "general": 2, "count": 4}                       # groups per LDS stage: ranges are whole stages
NAMED_PAIR = {"consensus": (1, 2), "general": (4, 5), "count": (1, 2)}          # the pair whose unsplit sum passes 2^24

_BASES = np.frombuffer(b"ACGT", np.uint8)
_PARTIAL = np.frombuffer(b"MRWSYKVHDB", np.uint8)
_N = ord("N")

# IUPAC letter -> allele set (bit 0 = A, 1 = C, 2 = G, 3 = T); every other byte is fully ambiguous, as the packer reads it
MASK_OF = np.full(256, 15, np.uint8)
for _ch, _m in zip(b"ACGTMRWSYKVHDB", (1, 2, 4, 8, 3, 5, 9, 6, 10, 12, 7, 11, 13, 14)):
    MASK_OF[_ch] = MASK_OF[_ch + 32] = _m


def _hit(rng, L, p):
    return rng.random(L, dtype=np.float32) < np.float32(p)


def _substituted(base, rng, p):
    """base (indices 0..3) with another base at a fraction p of the sites"""
    out = base.copy()
    sel = np.flatnonzero(_hit(rng, base.size, p))
    out[sel] = (out[sel] + rng.integers(1, 4, sel.size, dtype=np.uint8)) & 3
    return out


def _row(base, rng, mask=None, p_n=0.01):
    row = _BASES[base]
    if mask is not None:
        row[mask] = _N
    if p_n:
        row[_hit(rng, base.size, p_n)] = _N
    return row


def shared_mask(L, fraction):
    """The fixed mask M: `fraction` of the sites, the same for every caller"""
    return _hit(np.random.default_rng(7500 + int(round(fraction * 100))), L, fraction)


def consensus_rows(L=L_PAIR, seed=2201):
    """n = 6, A/C/G/T/N only.  Row 0 random; 1 = row 0 with 1e-3 substitutions and 1 % N of its own; 2 = row 0 with 1 % N; 3 = another
    base than row 0 at every site, 1 % N; 4 = row 0 with N on M (75 % of the sites) and 1 % N of its own; 5 = as 4, with 1e-3 substitutions."""
    rng = np.random.default_rng(seed)
    b0 = rng.integers(0, 4, L, dtype=np.uint8)
    M = shared_mask(L, 0.75)
    rows = [_row(b0, rng, p_n=0.0),
            _row(_substituted(b0, rng, 1e-3), rng),
            _row(b0, rng),
            _row((b0 + rng.integers(1, 4, L, dtype=np.uint8)) & 3, rng),
            _row(b0, rng, M),
            _row(_substituted(b0, rng, 1e-3), rng, M)]
    return np.array(rows)


GENERAL_DISTINCT = 7                      # rows 0..6 of general_rows hold every distinct row: the others are copies of row 0, as row 6 is


def general_rows(L=L_PAIR, seed=2201):
    """n = 14: consensus_rows with partial IUPAC codes at rate 1e-4 in rows 1 and 2, and eight copies of row 0 behind them.  The general
    route keeps a per-sample list of every N site as well and refuses lists of more than one entry per 8 sites of the whole alignment
    (general_sparse.hip: gs_build's max_entries = n L / 8) -- the VALU kernel runs then.  Rows 4 and 5 alone are 1.5 L entries, the six
    rows 1.54 L: n L / 8 > 1.54 L needs n >= 13.  The copies carry no N: with n = 14 the lists fill 88 % of the cap."""
    six = consensus_rows(L, seed)
    rng = np.random.default_rng(seed + 1)
    for r in (1, 2):
        sel = np.flatnonzero(_hit(rng, L, 1e-4))
        six[r, sel] = _PARTIAL[rng.integers(0, len(_PARTIAL), sel.size)]
    return np.concatenate([six, np.repeat(six[:1], 8, axis=0)])


def count_rows(L=L_COUNT, seed=2203):
    """n = 3.  Row 0 random A/C/G/T; rows 1 and 2 = row 0 with N on one shared mask of 95 % of the sites, plus 1 % N of their own: no
    site separates two samples (every d is 0, no dense site), 95 % of the sites hold a pair of N samples."""
    rng = np.random.default_rng(seed)
    b0 = rng.integers(0, 4, L, dtype=np.uint8)
    M = shared_mask(L, 0.95)
    return np.array([_row(b0, rng, p_n=0.0), _row(b0, rng, M), _row(b0, rng, M)])


BUILDERS = {"consensus": consensus_rows, "general": general_rows, "count": count_rows}


def pairs(n):
    """(i, j) of every pair j > i, row-major"""
    i, j = np.triu_indices(n, 1)
    return i, j


def reference(seqs):
    """-> d, nn (int64, pairs(n) order) straight from the 4-bit allele sets: d = #(m_i & m_j == 0), nn = L - #(m_i == 15 or m_j == 15)"""
    m = MASK_OF[seqs]
    L = seqs.shape[1]
    isn = m == 15
    ri, ci = pairs(len(seqs))
    d = np.array([np.count_nonzero((m[i] & m[j]) == 0) for i, j in zip(ri, ci)], np.int64)
    nn = np.array([L - np.count_nonzero(isn[i] | isn[j]) for i, j in zip(ri, ci)], np.int64)
    return d, nn


_POP4 = np.array([bin(v).count("1") for v in range(16)], np.int64)


def precondition_value(kind, seqs):
    """The named pair's sum over the whole alignment, the one an unsplit range would hold in one fp32 accumulator:
    consensus 4 * matches - nn, general sum |S_i n S_j|, count #(both N)."""
    m = MASK_OF[seqs]
    i, j = NAMED_PAIR[kind]
    if kind == "consensus":
        both = (m[i] != 15) & (m[j] != 15)
        return 4 * int(np.count_nonzero(both & (m[i] == m[j]))) - int(np.count_nonzero(both))
    if kind == "general":
        return int(np.bincount(m[i] & m[j], minlength=16) @ _POP4)
    return int(np.count_nonzero((m[i] == 15) & (m[j] == 15)))


def assert_precondition(kind, seqs):
    v = precondition_value(kind, seqs)
    assert v > (1 << 24), "%s case no longer tests the bound: the sum of pair %s is %d <= 2^24" % (kind, NAMED_PAIR[kind], v)
    return v


def groups_of(L):
    return (L + SITES_PER_GROUP - 1) // SITES_PER_GROUP


def forced_prefix(kind, L=L_PAIR):
    """The largest stage-aligned number of groups below the alignment's: what TRACS_THR_PREFIX is forced to (49 152 at L_PAIR)"""
    gc = STAGE_GROUPS[kind]
    return (groups_of(L) - 1) // gc * gc
