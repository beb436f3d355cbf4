"""The restatement of the bootstrap definitions (tests/bootstrap_ref.py) against answers worked out once with Python
integers, and its own invariants.  No GPU, no library."""
import numpy as np
import pytest

import bootstrap_ref as br
import nj_ref


def test_mix_is_the_splitmix64_finaliser():
    # splitmix64 seeded with 0 gives these first outputs: mix(G), mix(2 G)
    assert br.mix(br.GOLDEN) == 0xE220A8397B1DCDAF
    assert br.mix((2 * br.GOLDEN) & br.M64) == 0x6E789E6AA1B965F4
    assert br.mix(0) == 0 and br.mix(1) == 0x5692161D100B05E5
    assert br.key(1, 0) == 0x910A2DEC89025CC1


# (S, b, t, L) -> u, c: worked out once with Python integers
KNOWN = [
    ((1, 0, 0, 1), 0x5E41AB087439611E, 0),                                # L = 1: always column 0
    ((1, 0, 0, 2 ** 32 - 1), 0x5E41AB087439611E, 1581361928),
    ((1, 0, 1, 2 ** 32 - 1), 0xF18D6CE93D6CF1EE, 4052577512),              # u with its top bit set: the product needs all 128 bits
    ((3, 7, 5, 600), 0xC07B259322BAFBFC, 451),
    ((0, 0, 0, 4133), 0xA706DD2F4D197E6F, 2696),
    ((2 ** 64 - 1, 2, 129, 129), 0x34608A2921FD0700, 26),                 # the seed wraps mod 2^64
    ((1, 7, 4132, 4133), 0x23F18BA5F149A0C6, 580),
    ((12345678901234567890, 1, 0, 5000000), 0x7D55319E0E82A4A7, 2447906),
]


@pytest.mark.parametrize("args,u,c", KNOWN, ids=[str(k[0]) for k in KNOWN])
def test_known_answer_draws(args, u, c):
    S, b, t, L = args
    assert br.u(S, b, t) == u
    assert br.draw(S, b, t, L) == c == (u * L) >> 64 and 0 <= c < L


def test_a_wrong_high_half_would_show():
    """the signed or 64-bit-only products differ from the definition on the case with the top bit set"""
    u, L = 0xF18D6CE93D6CF1EE, 2 ** 32 - 1
    assert ((u * L) & br.M64) >> 32 != (u * L) >> 64
    assert (((u - (1 << 64)) * L) >> 64) % (1 << 64) != (u * L) >> 64


@pytest.mark.parametrize("L", [1, 2, 31, 128, 129, 600, 4133])
def test_weights_sum_to_L(L):
    for seed, b in ((1, 0), (3, 7), (2 ** 64 - 1, 1)):
        w = br.weights(L, seed, b)
        assert w.dtype == np.int64 and w.shape == (L,) and int(w.sum()) == L and w.min() >= 0
        counts = np.bincount([br.draw(seed, b, t, L) for t in range(L)], minlength=L)
        assert np.array_equal(counts, w)


def test_seeds_and_replicates_differ():
    L = 600
    w = {(s, b): br.weights(L, s, b) for s in (1, 3) for b in (0, 1)}
    keys = list(w)
    for i in range(len(keys)):
        for j in range(i + 1, len(keys)):
            assert not np.array_equal(w[keys[i]], w[keys[j]]), (keys[i], keys[j])
    assert np.array_equal(w[(1, 0)], br.weights(L, 1, 0))                   # and a replicate is a function of (L, seed, b) alone
    # about 1 / e of the columns are not drawn, and some are drawn more than twice
    assert 0.3 < (w[(1, 0)] == 0).mean() < 0.45 and w[(1, 0)].max() >= 3


def test_repeated_text_and_weighted_distances():
    rng = np.random.default_rng(5)
    seqs = rng.choice(np.frombuffer(b"ACGTNRYacgt-", np.uint8), (7, 40))
    w = br.weights(40, 9, 2)
    rep = br.repeated(seqs, w)
    assert rep.shape == (7, 40) and np.array_equal(rep[:, :w[0]], np.repeat(seqs[:, :1], w[0], axis=1))
    assert np.array_equal(br.snp_matrix(rep), br.snp_matrix(seqs, w))        # d_b = the sum of w_b over the disjoint columns
    D = br.snp_matrix(seqs)
    assert np.array_equal(D, D.T) and not D.diagonal().any()
    # columns at which no two samples differ add nothing
    dif = br.differs(seqs)
    w2 = w.copy()
    w2[~dif] = 0
    assert np.array_equal(br.snp_matrix(seqs, w2), br.snp_matrix(seqs, w))
    assert np.array_equal(br.canonical(np.frombuffer(b"ACGTNn-RrX", np.uint8)), np.frombuffer(b"ACGTNNNRRN", np.uint8))


def test_supports_of_known_trees():
    rng = np.random.default_rng(2)
    for n in (4, 5, 6, 9, 65):
        main = br.random_tree_edges(n, rng)
        sp = br.internal_splits(n, *main)
        assert len(sp) == n - 3 and all(not (m & 1) and bin(m).count("1") >= 2 for m in sp)
        assert set(sp) <= set(nj_ref.splits_of(n, main[0], main[1], np.zeros(len(main[0]))))
        s = br.supports(n, main, [main, main])
        assert ((s == 2) == (main[1] >= n)).all() and ((s == br.NONE) == (main[1] < n)).all()
    # ((0,1),(2,3),4...) against a tree that shares exactly one split
    main = (np.array([5, 5, 6, 6, 7, 7, 7], np.uint32), np.array([0, 1, 2, 3, 4, 5, 6], np.uint32))         # splits {0,1} -> {2,3,4}, {2,3}
    other = (np.array([5, 5, 6, 6, 7, 7, 7], np.uint32), np.array([0, 1, 2, 4, 3, 5, 6], np.uint32))        # splits {2,3,4}, {2,4}
    assert br.supports(5, main, [other]).tolist() == [br.NONE] * 5 + [1, 0]
    assert (br.supports(3, (np.array([3, 3, 3]), np.array([0, 1, 2])), []) == br.NONE).all()
    cat = br.caterpillar_edges(list(range(6)))
    assert sorted(br.internal_splits(6, *cat)) == sorted([0b111100, 0b111000, 0b110000])


def test_the_end_to_end_fixture_is_not_degenerate():
    """what tests/test_gpu_bootstrap.py runs through the command line (--bootstrap 8 --bootstrap-seed 3), on the restatement alone: some
    support equals B, some lies strictly between 0 and B, and the 40-column clade is one of the former"""
    seqs = br.outbreak_alignment()
    n, B, seed = 24, 8, 3
    assert seqs.shape == (n, 600) and np.array_equal(seqs[22], seqs[23])
    assert (br.MASKS[seqs] == 15).any() and np.isin(br.MASKS[seqs], (5, 10)).any()                 # N and partial codes
    main = nj_ref.nj(br.snp_matrix(seqs).astype(np.float64))
    reps = [br.replicate_tree(seqs, seed, b) for b in range(B)]
    s = br.supports(n, main, reps)
    inner = s[main[1] >= n]
    assert len(inner) == n - 3 and (s[main[1] < n] == br.NONE).all()
    assert (inner == B).any() and ((inner > 0) & (inner < B)).any() and inner.max() <= B
    clade = sum(1 << k for k in range(8, 24))                               # samples 0 .. 7 against the rest, on the side without leaf 0
    assert s[br.internal_splits(n, main[0], main[1])[clade]] == B
    other = [br.replicate_tree(seqs, 4, b) for b in range(B)]
    assert any(not np.array_equal(a[2], b[2]) for a, b in zip(reps, other))
