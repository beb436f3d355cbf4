"""The key-table transcluster route (device.trans_dist_dense_partitioned: tracs_trans_table_dense -> all-reduce of the tables ->
tracs_trans_table_gather; what bench.py runs when world > 1) on one GPU, the ranks played one after the other in this process:
P / E(K) of every rank BIT-EQUAL to the single call over the whole matrix (tracs_trans_dist_dense2), every distinct (N, day gap) key
written into the table by exactly one hash class, the overflow flag of a table that is too small, and the row / column bounds of the
two C entry points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_keysplit import _matrix  # noqa: E402

pytestmark = pytest.mark.gpu

LAMB, BETA, PREC = 5.3, 6.0, 0.01
BIG = 2147483647
FILL = float("nan")
SENTINEL = 0x7FF8DEADBEEF0001                      # a NaN no kernel produces: "this table slot was not written"

# (n, parts): 257 / 500 / 1000 with every split, and 40 samples over 8 classes (some classes without a key)
SPLITS = [(n, parts) for n in (257, 500, 1000) for parts in (1, 2, 3, 8)] + [(40, 8)]


def _case(n):
    return _matrix(n, 11 + n, spread=400 if n == 1000 else 40)


def _padded(a, ld, pad):
    """a ([n, n] numpy) as the first n columns of a [n, ld] device buffer (columns n.. hold `pad`) -> (buffer, view [n, n])"""
    import torch
    n = a.shape[0]
    t = torch.from_numpy(a).cuda()
    buf = torch.full((n, ld), pad, dtype=t.dtype, device="cuda")
    buf[:, :n] = t
    return buf, buf[:, :n]


def _nan_pair(n, ld):
    """two NaN-filled [n, ld] float64 buffers and their [n, n] views"""
    import torch
    bufs = [torch.full((n, ld), FILL, dtype=torch.float64, device="cuda") for _ in range(2)]
    return bufs, [b[:, :n] for b in bufs]


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


def _keys(d, days, thr, row_begin=0, row_end=None, col_begin=0):
    """numpy: the valid cells' (N, |day gap|) and the mask of the valid cells"""
    n = d.shape[0]
    row_end = n if row_end is None else row_end
    i, j = np.mgrid[0:n, 0:n]
    valid = (j > i) & (j >= col_begin) & (i >= row_begin) & (i < row_end) & (d.astype(np.int64) <= thr)
    gap = np.abs(days.astype(np.int64)[:, None] - days.astype(np.int64)[None, :])
    return d.astype(np.int64)[valid], gap[valid], valid


def play_parts(dev, dist, n, days, lamb, beta, prec, parts, exp_p0, dist_threshold, ld, n_max=None, d_max=None):
    """The ranks of trans_dist_dense_partitioned one after the other.  Round one: every part's all_reduce only clones the table it is
    given (that part's keys, zeros elsewhere).  Round two: all_reduce copies the SUM of the cloned tables into its argument -- what the
    all-reduce over the ranks does -- and the part gathers.  -> [(P buffer, E(K) buffer)] of round two, one pair of [n, ld] buffers
    per part, NaN where nothing was written."""
    import torch
    clones = []
    if parts > 1:
        for p in range(parts):
            _, (ps, es) = _nan_pair(n, ld)
            dev.trans_dist_dense_partitioned(dist, n, days, lamb, beta, prec, ps, es, part=p, parts=parts,
                                             all_reduce=lambda t: clones.append(t.clone()), exp_p0=exp_p0,
                                             dist_threshold=dist_threshold, n_max=n_max, d_max=d_max)
        assert len(clones) == parts
    out = []
    for p in range(parts):
        bufs, (pv, ev) = _nan_pair(n, ld)
        dev.trans_dist_dense_partitioned(dist, n, days, lamb, beta, prec, pv, ev, part=p, parts=parts,
                                         all_reduce=lambda t: t.copy_(torch.stack(clones).sum(0)), exp_p0=exp_p0,
                                         dist_threshold=dist_threshold, n_max=n_max, d_max=d_max)
        out.append(tuple(bufs))
    return out


@pytest.mark.parametrize("thr", [BIG, 100])
@pytest.mark.parametrize("n,parts", SPLITS)
def test_partitioned_equals_the_single_call(n, parts, thr):
    """ld = n and n + 3 (for n = 257 and 1000: ld % 4 != 0 and == 0, the scalar and the 8-byte paths of tc_for_row_quads and
    tc_table_gather2_kernel), exp_p0 both ways."""
    import torch
    from tracs_amd import device as dev
    d, days = _case(n)
    N, gap, valid = _keys(d, days, thr)
    distinct = len(set(zip(N.tolist(), gap.tolist())))
    dy = torch.from_numpy(days).cuda()
    for ld in (n, n + 3):
        _, dm = _padded(d, ld, 5)                                      # (the padding columns look like cells within the threshold)
        vpad = np.zeros((n, ld), bool)
        vpad[:, :n] = valid
        for exp_p0 in (True, False):
            base, (p1, e1) = _nan_pair(n, ld)
            dev.trans_dist_dense_ranges(dm, n, dy, LAMB, BETA, PREC, p1, e1, [(0, n)], exp_p0=exp_p0, dist_threshold=thr)
            r1 = dev.trans_routes()
            want = [_bits(b) for b in base]
            # the baseline itself: a value in every valid cell, the fill everywhere else
            for b in base:
                assert np.array_equal(~np.isnan(b.cpu().numpy()), vpad)
            assert r1["keys"] == distinct
            got = play_parts(dev, dm, n, dy, LAMB, BETA, PREC, parts, exp_p0, thr, ld)
            # The route counters after a partitioned call: `keys` counts the distinct keys of ALL hash classes (the dedup runs before
            # the split) and `tables` is decided from them, so both must agree with the single call; the per-kernel counters also
            # count the other classes' keys (they leave tc_keys_kernel as if done), so nothing is asserted on them.
            r2 = dev.trans_routes()
            assert r2["keys"] == distinct and r2["route"] == "hash" and r2["tables"] == r1["tables"], (r1, r2)
            if n == 1000:
                assert distinct >= 2048 and r2["tables"], r2            # the prefix tables are reached
            for p, (pb, eb) in enumerate(got):
                assert np.array_equal(_bits(pb), want[0]), "P of part %d of %d (ld %d, exp_p0 %s)" % (p, parts, ld, exp_p0)
                assert np.array_equal(_bits(eb), want[1]), "E(K) of part %d of %d (ld %d, exp_p0 %s)" % (p, parts, ld, exp_p0)


def test_inputs_reach_the_wave_and_ratio_kernels():
    """A coverage condition on the INPUT (numpy only): the 1000-sample case has keys with N >= 128 (tc_keys_kernel's
    TC_WAVE_PREFIX_MIN: handed to the ratio / wave kernels) both on the same day and on different days, and at least 2 048 distinct
    keys (the gate of the prefix tables) within either threshold."""
    d, days = _case(1000)
    N, gap, _ = _keys(d, days, BIG)
    assert ((N >= 128) & (gap == 0)).any() and ((N >= 128) & (gap > 0)).any()
    for thr in (BIG, 100):
        N, gap, _ = _keys(d, days, thr)
        assert len(set(zip(N.tolist(), gap.tolist()))) >= 2048


def _table_dense(dev, L, dm, ld, n, dy, thr, part, parts, n_max, d_max, tp, te, flag, rows=None, col_begin=0):
    from tracs_amd import _lib
    r0, r1 = rows if rows is not None else (0, n)
    _lib.check(L.tracs_trans_table_dense(dev._ptr(dm), ld, n, r0, r1, col_begin, int(thr), dev._ptr(dy), LAMB, BETA, PREC, part, parts,
                                         n_max, d_max, dev._ptr(tp), dev._ptr(te), dev._ptr(flag), dev._stream()))


@pytest.mark.parametrize("thr", [BIG, 100])
@pytest.mark.parametrize("n,parts", SPLITS)
def test_every_key_is_written_by_exactly_one_part(n, parts, thr):
    """tracs_trans_table_dense itself, each part into its own sentinel-filled tables: the parts' written slots are pairwise disjoint,
    their union is exactly the slots N (d_max + 1) + gap of the valid cells' distinct keys, and a written slot has both values."""
    import torch
    from tracs_amd import _lib
    from tracs_amd import device as dev
    L = _lib.load()
    d, days = _case(n)
    N, gap, _ = _keys(d, days, thr)
    n_max, d_max = int(N.max()), int(days.max()) - int(days.min())
    cells = (n_max + 1) * (d_max + 1)
    want = np.zeros(cells, bool)
    want[N * (d_max + 1) + gap] = True
    distinct = int(want.sum())
    dy = torch.from_numpy(days).cuda()
    for ld in (n, n + 3):
        _, dm = _padded(d, ld, 5)
        times = np.zeros(cells, np.int32)
        for p in range(parts):
            tp = torch.full((cells,), SENTINEL, dtype=torch.int64, device="cuda").view(torch.float64)
            te = torch.full((cells,), SENTINEL, dtype=torch.int64, device="cuda").view(torch.float64)
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            _table_dense(dev, L, dm, ld, n, dy, thr, p, parts, n_max, d_max, tp, te, flag)
            wp, we = _bits(tp) != SENTINEL, _bits(te) != SENTINEL
            assert int(flag.item()) == 0
            assert np.array_equal(wp, we), "part %d: %d slots with only one of p0 / E(K)" % (p, int((wp != we).sum()))
            assert not (wp & ~want).any(), "part %d wrote %d slots that are no key of the matrix" % (p, int((wp & ~want).sum()))
            if distinct >= 2048:
                assert wp.any(), "part %d of %d evaluated nothing" % (p, parts)
            times += wp
        assert int(times.max()) <= 1, "%d keys written by more than one part" % int((times > 1).sum())
        assert np.array_equal(times == 1, want), "%d keys written by no part" % int((want & (times == 0)).sum())


def test_a_table_too_small_is_reported():
    """n_max one below the largest valid distance, or d_max one below the largest valid gap: TracsError, from whichever part is
    asked; the exact bounds: no error.  The matrix's largest distance (129) lies ABOVE the threshold: those cells must not count."""
    import torch
    from tracs_amd import _lib
    from tracs_amd import device as dev
    n, thr = 257, 100
    d, days = _case(n)
    N, gap, _ = _keys(d, days, thr)
    n_max, d_max = int(N.max()), int(gap.max())
    assert int(np.triu(d, 1).max()) > thr >= n_max and d_max >= 1
    dm, dy = torch.from_numpy(d).cuda(), torch.from_numpy(days).cuda()

    def run(part, parts, nm, dmx):
        _, (p, e) = _nan_pair(n, n)
        dev.trans_dist_dense_partitioned(dm, n, dy, LAMB, BETA, PREC, p, e, part=part, parts=parts, all_reduce=lambda t: None,
                                         dist_threshold=thr, n_max=nm, d_max=dmx)

    for parts in (1, 3):
        for part in range(parts):
            run(part, parts, n_max, d_max)
            with pytest.raises(_lib.TracsError, match="key table"):
                run(part, parts, n_max - 1, d_max)
            with pytest.raises(_lib.TracsError, match="key table"):
                run(part, parts, n_max, d_max - 1)


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("thr", [BIG, 100])
def test_row_and_column_bounds(thr, parts):
    """tracs_trans_table_dense / _gather over rows [100, 333), columns >= 64 of 500 samples = trans_dist_dense_ranges with the same
    bounds, bit for bit; nothing outside those cells is written."""
    import torch
    from tracs_amd import _lib
    from tracs_amd import device as dev
    L = _lib.load()
    n, rows, cb = 500, (100, 333), 64
    d, days = _case(n)
    N, gap, valid = _keys(d, days, thr, rows[0], rows[1], cb)
    n_max, d_max = int(N.max()), int(gap.max())
    cells = (n_max + 1) * (d_max + 1)
    dy = torch.from_numpy(days).cuda()
    for ld in (n, n + 3):
        _, dm = _padded(d, ld, 5)
        vpad = np.zeros((n, ld), bool)
        vpad[:, :n] = valid
        base, (p1, e1) = _nan_pair(n, ld)
        dev.trans_dist_dense_ranges(dm, n, dy, LAMB, BETA, PREC, p1, e1, [rows], exp_p0=True, dist_threshold=thr, col_begin=cb)
        assert np.array_equal(~np.isnan(base[0].cpu().numpy()), vpad) and np.array_equal(~np.isnan(base[1].cpu().numpy()), vpad)
        table = torch.zeros((2, cells), dtype=torch.float64, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        for p in range(parts):                                         # (the all-reduce: every part's table summed)
            t = torch.zeros_like(table)
            _table_dense(dev, L, dm, ld, n, dy, thr, p, parts, n_max, d_max, t[0], t[1], flag, rows, cb)
            table += t
        got, (p2, e2) = _nan_pair(n, ld)
        _lib.check(L.tracs_trans_table_gather(dev._ptr(dm), ld, n, rows[0], rows[1], cb, int(thr), dev._ptr(dy), n_max, d_max,
                                              dev._ptr(table[0]), dev._ptr(table[1]), 1, dev._ptr(p2), dev._ptr(e2), dev._ptr(flag),
                                              dev._stream()))
        assert int(flag.item()) == 0
        assert np.array_equal(_bits(got[0]), _bits(base[0])) and np.array_equal(_bits(got[1]), _bits(base[1]))
