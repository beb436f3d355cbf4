"""The inputs of tests/test_gpu_exact_range.py discriminate: under a model of the matrix-core kernels' fp32 accumulators
(tests/fp32_range_model.py) every case is exact with ranges at the host code's bound and inexact with one range over the whole
alignment.  No GPU: this is what shows that the GPU tests would fail if a bound of csrc/pairsnp.hip were dropped."""
import numpy as np
import pytest

import exact_range_cases as X
import fp32_range_model as F

CASES = ["consensus", "general", "count-in-place", "count-repacked"]


@pytest.fixture(scope="module", params=CASES)
def case(request):
    kind = request.param.split("-")[0]
    seqs = _distinct(kind, X.BUILDERS[kind]())
    X.assert_precondition(kind, seqs)
    d, nn = X.reference(seqs)
    if kind == "consensus":
        model = F.ConsensusModel(seqs)
    elif kind == "general":
        model = F.GeneralModel(seqs, d)
    else:
        model = F.CountModel(seqs, in_place=request.param == "count-in-place")
    groups = model.groups if kind == "count" else X.groups_of(seqs.shape[1])
    return kind, seqs, d, nn, model, groups


def _distinct(kind, seqs):
    """the general case without its repeated rows (copies of row 0, as row 6 is): every distinct pair is still there"""
    if kind == "general":
        assert (seqs[X.GENERAL_DISTINCT:] == seqs[0]).all()
        return seqs[:X.GENERAL_DISTINCT]
    return seqs


def _modelled(kind, model, n, bounds):
    """-> d, nn of every pair (None for the counting form's d: it is not that pass's)"""
    if kind == "count":
        return None, np.array([model.pair_nn(i, j, bounds) for i, j in zip(*X.pairs(n))], np.int64)
    out = [model.pair(i, j, bounds) for i, j in zip(*X.pairs(n))]
    return np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.int64)


def test_float32_accumulate_is_sequential():
    """np.add.accumulate in float32 rounds after every addition: 2^24 + 1 + 1 stays 2^24, and 3 goes to 4 on the way"""
    assert F.f32_ranges(np.array([1 << 24, 1, 1]), 1, [0, 3]) == [1 << 24]
    assert F.f32_ranges(np.array([1 << 24, 3, 3]), 1, [0, 3]) == [(1 << 24) + 8]
    assert F.f32_ranges(np.array([1 << 24, 1, 1]), 1, [0, 1, 3]) == [1 << 24, 2]


def test_exact_with_ranges_at_the_bound(case):
    """a) ranges of 2^22 (consensus), 2^21 (general), 2^23 (count) sites: the modelled d and nn are the reference's, every pair"""
    kind, seqs, d, nn, model, groups = case
    bounds = F.range_bounds(groups, X.BOUND_SITES[kind] // X.SITES_PER_GROUP)
    assert len(bounds) > 2, "one range would do: the case does not reach the bound"
    md, mnn = _modelled(kind, model, len(seqs), bounds)
    assert np.array_equal(mnn, nn)
    assert md is None or np.array_equal(md, d)


def test_inexact_with_one_range(case):
    """b) one range over the whole alignment: the named pair's d or nn is off -- the input tells a missing bound from a right one"""
    kind, seqs, d, nn, model, groups = case
    md, mnn = _modelled(kind, model, len(seqs), [0, groups])
    k = list(zip(*X.pairs(len(seqs)))).index(X.NAMED_PAIR[kind])
    off_d, off_nn = (0 if md is None else int(md[k] - d[k])), int(mnn[k] - nn[k])
    print("%s, one range: pair %s d off by %d, nn off by %d" % (kind, X.NAMED_PAIR[kind], off_d, off_nn))
    assert off_d != 0 or off_nn != 0


@pytest.mark.parametrize("kind", ["consensus", "general"])
def test_forced_prefix_range(kind):
    """The thresholded two-pass run with TRACS_THR_PREFIX forced to 49 152 groups: as ONE prefix range (thr_prefix_groups without the
    clamp on a forced value) the named pair is off; clamped to the bound, with the remainder behind it, it is exact."""
    seqs = _distinct(kind, X.BUILDERS[kind]())
    d, nn = X.reference(seqs)
    model = F.ConsensusModel(seqs) if kind == "consensus" else F.GeneralModel(seqs, d)
    groups, prefix = X.groups_of(seqs.shape[1]), X.forced_prefix(kind)
    assert prefix == 49152 and groups == 49153
    i, j = X.NAMED_PAIR[kind]
    k = list(zip(*X.pairs(len(seqs)))).index((i, j))
    pd, pnn = model.pair(i, j, [0, prefix, groups])
    print("%s, one prefix range of %d groups: pair (%d, %d) d off by %d, nn off by %d" % (kind, prefix, i, j, pd - d[k], pnn - nn[k]))
    assert (pd, pnn) != (int(d[k]), int(nn[k]))
    clamped = X.BOUND_SITES[kind] // X.SITES_PER_GROUP
    assert model.pair(i, j, [0, clamped, groups]) == (int(d[k]), int(nn[k]))
