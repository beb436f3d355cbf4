"""Neighbour joining on the device (tracs_nj_*: csrc/nj.hip, through tracs_amd.device) against the definition restated in numpy
(tests/nj_ref.py).  Every comparison is bit for bit: the joined nodes as integers, D_ab and the row sums as uint64 views."""
import functools

import numpy as np
import pytest

import nj_ref

pytestmark = pytest.mark.gpu

SIZES = [3, 4, 5, 63, 64, 65, 257, 520]       # a row shorter than / equal to / longer than a wave, more than one workgroup in the scan
KINDS = ["ints", "equal", "zero", "tree"]


@functools.lru_cache(maxsize=None)
def matrix(n, kind):
    rng = np.random.default_rng(17 * n + len(kind))
    if kind == "ints":                             # {0..3}: ties everywhere
        U = np.triu(rng.integers(0, 4, (n, n)), 1)
        D = (U + U.T).astype(np.float64)
    elif kind == "equal":
        D = 5.0 * (np.ones((n, n)) - np.eye(n))
    elif kind == "zero":
        D = np.zeros((n, n))
    else:
        D = nj_ref.random_tree_metric(n, rng)[0]
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def reference(n, kind):
    return nj_ref.nj_records(matrix(n, kind))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def assert_same(got, want, what):
    (a, b, dab, ra, rb), ids, d = got
    (wa, wb, wdab, wra, wrb), wids, wd = want
    assert np.array_equal(a, wa) and np.array_equal(b, wb), (what, np.flatnonzero((a != wa) | (b != wb))[:5])
    for name, x, y in (("D_ab", dab, wdab), ("R_a", ra, wra), ("R_b", rb, wrb)):
        assert np.array_equal(bits(x), bits(y)), (what, name, np.flatnonzero(bits(x) != bits(y))[:5])
    assert np.array_equal(ids, wids), (what, ids, wids)
    assert np.array_equal(bits(d), bits(wd)), (what, d, wd)


def run_f64(D, pad=0):
    import torch

    from tracs_amd import device as dev
    n = D.shape[0]
    M = torch.full((n, n + pad), -1.0, dtype=torch.float64)
    M[:, :n] = torch.from_numpy(np.array(D))
    state = dev.nj_init(n)
    if n >= 2:                                     # (below that there is no cell to load)
        dev.nj_load_f64(state, n, M.cuda())
    dev.nj_run(state, n)
    return dev.nj_emit(state, n)


def run_panels(d, nn, bounds, pad=0, per_site=False):
    """d, nn: integer n x n; only the cells j > i are handed over (the rest is poisoned), in the row panels bounds[k] .. bounds[k + 1]"""
    import torch

    from tracs_amd import device as dev
    n = d.shape[0]
    state = dev.nj_init(n)
    upper = np.triu(np.ones((n, n), bool), 1)
    for r0, r1 in zip(bounds[:-1], bounds[1:]):
        pd = np.full((r1 - r0, n + pad), 0x7FFFFFF0, np.int64)
        pn = np.zeros((r1 - r0, n + pad), np.int64)
        pd[:, :n] = np.where(upper[r0:r1], d[r0:r1], 0x7FFFFFF0)
        pn[:, :n] = np.where(upper[r0:r1], nn[r0:r1] if nn is not None else 1, 0)
        td = torch.from_numpy(pd.astype(np.uint32).view(np.int32)).cuda()
        tn = torch.from_numpy(pn.astype(np.uint32).view(np.int32)).cuda() if (nn is not None or per_site) else None
        dev.nj_load_panel(state, n, td, tn, row_begin=r0, row_end=r1, per_site=per_site, base_row=r0)
    dev.nj_run(state, n)
    return dev.nj_emit(state, n)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_records_equal_the_definition_bit_for_bit(hiplib, n, kind):
    assert_same(run_f64(matrix(n, kind)), reference(n, kind), (n, kind))


@pytest.mark.parametrize("n,kind", [(65, "ints"), (257, "ints"), (64, "tree")])
def test_panels_in_any_split_and_with_a_wider_leading_dimension(hiplib, n, kind):
    d = matrix(n, kind).astype(np.int64)
    want = reference(n, kind)
    assert_same(run_panels(d, None, [0, n], pad=7), want, "ld = n + 7")
    assert_same(run_panels(d, None, [0, n // 3, n]), want, "two panels")
    assert_same(run_panels(d, None, [0, 1, n // 4, n // 2, n - 2, n], pad=7), want, "five panels")
    assert_same(run_f64(matrix(n, kind), pad=7), want, "f64, ld = n + 7")


def test_small_n_and_a_state_is_run_once(hiplib):
    from tracs_amd import device as dev
    for n in (0, 1, 2):
        D = 7.0 * (np.ones((n, n)) - np.eye(n))
        assert_same(run_f64(D), nj_ref.nj_records(D), n)
    state = dev.nj_init(5)
    with pytest.raises(RuntimeError, match="has not been run"):
        dev.nj_emit(state, 5)
    dev.nj_run(state, 5)
    with pytest.raises(RuntimeError, match="has been run"):
        dev.nj_run(state, 5)
    with pytest.raises(RuntimeError, match="another vertex count"):
        dev.nj_emit(state, 6)


@pytest.fixture(scope="module")
def oracle_pairs(oracle):
    """the oracle's d and nn for 257 x 4 000 with N and partial codes, as dense integer matrices"""
    from tracs_amd import synth
    n = 257
    seqs = synth.alignment(n, 4000, seed=23, mu_lineage=4e-3, mu_sample=1e-3, p_n=0.03, p_partial=0.01)
    r, c, d, nn = oracle.pairsnp_arrays(seqs, n_threads=8)
    D, N = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    D[r.astype(np.int64), c.astype(np.int64)] = d
    N[r.astype(np.int64), c.astype(np.int64)] = nn
    return D + D.T, N + N.T


def test_oracle_distances(hiplib, oracle_pairs):
    d, nn = oracle_pairs
    want = nj_ref.nj_records(d.astype(np.float64))
    assert_same(run_panels(d, nn, [0, 100, 257]), want, "snp, panels")
    assert_same(run_f64(d.astype(np.float64)), want, "snp, f64")


def test_per_site_distances_and_a_pair_without_sites(hiplib, oracle_pairs):
    d, nn = oracle_pairs
    assert (nn[np.triu_indices(257, 1)] > 0).all()
    Q = np.zeros((257, 257))
    iu = np.triu_indices(257, 1)
    Q[iu] = d[iu].astype(np.float64) / nn[iu].astype(np.float64)
    Q = Q + Q.T
    assert_same(run_panels(d, nn, [0, 64, 257], per_site=True), nj_ref.nj_records(Q), "per-site")
    holes = nn.copy()
    for i, j in ((200, 3), (7, 100), (7, 42)):
        holes[i, j] = holes[j, i] = 0
    with pytest.raises(ValueError, match="samples 3 and 200 .* 0 sites") as e:
        run_panels(d, holes, [0, 64, 257], per_site=True)
    assert e.value.pair == (3, 200)                                    # the first such pair in (i, j) order
    assert_same(run_panels(d, holes, [0, 64, 257]), nj_ref.nj_records(d.astype(np.float64)), "snp does not read nn")


def test_tree_metric_comes_back(hiplib):
    from tracs_amd import device as dev
    n = 200
    D, want = nj_ref.random_tree_metric(n, np.random.default_rng(5))
    rec, ids, d = run_f64(D)
    parent, child, length = dev.nj_edges(n, rec, ids, d)
    assert len(parent) == 2 * n - 3
    assert nj_ref.splits_of(n, parent, child, length) == want          # every split and every length, as doubles
    rp, rc, rl = nj_ref.nj_edges(n, rec, ids, d)                        # the library's lengths are the definition's
    assert np.array_equal(parent, rp) and np.array_equal(child, rc) and np.array_equal(bits(length), bits(rl))


def test_scan_with_several_tiles_per_row_and_per_workgroup(hiplib):
    """n = 2 100: above 2 048 active nodes a folded row of the scan is more than one tile and the scan has more tiles than
    workgroups, so a workgroup strides over tiles -- the shape every large run has for most of its joins.  A tree metric needs no
    O(n^3) reference: every split and every length must be the generator's, and the joins of the first steps (all of them above
    2 048 nodes) are checked against the definition on the records themselves."""
    from tracs_amd import device as dev
    n = 2100
    D, want = nj_ref.random_tree_metric(n, np.random.default_rng(11))
    rec, ids, d = run_f64(D)
    parent, child, length = dev.nj_edges(n, rec, ids, d)
    assert len(parent) == 2 * n - 3
    assert nj_ref.splits_of(n, parent, child, length) == want
    # the first join, recomputed from the definition over all n (n - 1) / 2 pairs
    R = nj_ref.row_sums(D)
    Q = (float(n - 2) * D) - (R[:, None] + R[None, :])
    Q[np.tril_indices(n)] = np.inf
    i, j = divmod(int(np.argmin(Q)), n)
    assert (int(rec[0][0]), int(rec[1][0])) == (i, j)
    assert bits(rec[2][:1])[0] == bits(D[i, j:j + 1])[0] and bits(rec[3][:1])[0] == bits(R[i:i + 1])[0] and bits(rec[4][:1])[0] == bits(R[j:j + 1])[0]
