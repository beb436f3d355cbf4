"""The posterior filter's three routes (csrc/dmultinomial.hip posterior_code: the integer table below POST_TABLE_TOT = 4096, the f32
screen above it, the f64 guard band for the cells the screen calls uncertain) at their edges, and the coverage-profile and consensus
kernels on their own.

Expected masks are the oracle's (oracle.calculate_posteriors: the reference's own arithmetic) with the coverage rules applied as
tracs/align.py:599-613 does (test_align_stage._reference_sequence).  The row table holds, for every total class -- 0, 1, 2, 4, 5,
4094 .. 4097 around the table's edge, 65 535, 262 140 (the uint16 maximum) and, as uint32 only, 2^24 +- 1 and 4 (2^30 - 1) -- the
count patterns (t,0,0,0), (a,a,0,0), (a,a,a,a), (a,b,b,0), (a,b,b,c), (a,b,c,d) and (t-1,1,0,0) in all 24 allele orders.  Windows of
1, 2, 511, 512, 513, 1024 and 1537 sites of it (the tail kernel alone, whole rounds without a tail, an odd tail) go in as uint16 where
the rows fit and always as uint32.  Thresholds: the exact f64 posterior of one cell per total class, the doubles either side, 0.01
and 0.3, the cells taken from the uint16 table's rows as well as the uint32 table's.  Every code byte must equal the oracle's, the
unused high nibble of an odd L's last byte included.  14 392 calls over the four alpha sets; on an MI355X no test of the module takes above
0.2 s.

Mutation, built and run once and then reverted: POST_TABLE_TOT lowered by one in posterior_code's comparison alone (the table keeps
its size), so that total 4095 takes the f32 screen and its guard band instead of the table.  Every test of this module still passes,
and so does test_gpu_golden.py::test_posterior_codes_on_the_threshold: with thresholds that are exact posteriors of cells at total
4095 (and the doubles either side) in every allele order, the screen with its f64 guard band decides as the integer table does, so
the routes agree at their common edge -- the mutation is not a bug these tests miss, it moves a site between two routes that give
the same answer."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_align_stage import _LUT, _reference_sequence  # noqa: E402

pytestmark = pytest.mark.gpu

CUTS = (1, 2, 511, 512, 513, 1024, 1537)
TOTALS16 = (0, 1, 2, 4, 5, 4094, 4095, 4096, 4097, 65535, 262140)
TOTALS32 = ((1 << 24) - 1, (1 << 24) + 1, 4 * ((1 << 30) - 1))
ALPHAS = {"cli": [20.8156311152126, 4.38181182238621, 0.889048781117318, 0.1],
          "small_last": [14.25, 1.508, 0.108, 0.0038],
          "equal": [3.0, 3.0, 3.0, 3.0],
          "degenerate": [0.0, 0.0, 0.0, 1.0]}
MIN_COVS = (0, 5, 4096, 4097)
BANDS = (None, (2.0, 4.0), (2.5, 2.7), (4095.5, 4096.5), (-3.0, 0.5), (-3.0, -1.0))
RULES = tuple(itertools.product(MIN_COVS, BANDS))
_CODE_OF = np.zeros(256, np.uint8)
_CODE_OF[_LUT] = np.arange(16, dtype=np.uint8)


@pytest.fixture(scope="module")
def torch_mod(hiplib):
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def dev(torch_mod):
    from tracs_amd import device
    return device


def _patterns(t, cap):
    """the count patterns of total t whose counts all fit `cap`"""
    out = [(t, 0, 0, 0)]
    if t % 2 == 0:
        out.append((t // 2, t // 2, 0, 0))
    if t % 4 == 0:
        out.append((t // 4,) * 4)
    b = t // 4
    if b > 0 and t - 2 * b != b:
        out.append((t - 2 * b, b, b, 0))
    c = max(1, t // 16)
    if b > c and t - 2 * b - c > b:
        out.append((t - 2 * b - c, b, b, c))
    b, c, d = t // 4, t // 8, t // 16
    if t - b - c - d > b > c > d >= 0 and t >= 6:
        out.append((t - b - c - d, b, c, d))
    if t >= 2:
        out.append((t - 1, 1, 0, 0))
    return sorted(set(p for p in out if max(p) <= cap and sum(p) == t))


def _table(totals, cap):
    rows = [[p[i] for i in perm] for t in totals for p in _patterns(t, cap) for perm in itertools.permutations(range(4))]
    rows = np.array(rows, np.int64)
    return rows[np.random.default_rng(7).permutation(len(rows))]          # classes mixed, so that every window holds several


@pytest.fixture(scope="module")
def tables(torch_mod):
    """{"u16" / "u32": (int64 rows, [(offset, L, device tensor)])}: consecutive windows of the shuffled table, wrapping round, so that
    every row is in some window"""
    torch = torch_mod
    out = {}
    for name, rows in (("u16", _table(TOTALS16, 65535)), ("u32", _table(TOTALS16 + TOTALS32, (1 << 30) - 1))):
        assert set(rows.sum(1).tolist()) == set(TOTALS16 if name == "u16" else TOTALS16 + TOTALS32)
        cuts, off = [], 0
        for L in CUTS:
            idx = (off + np.arange(L)) % len(rows)
            narrow = rows[idx].astype(np.uint16).view(np.int16) if name == "u16" else rows[idx].astype(np.uint32).view(np.int32)
            cuts.append((idx, L, torch.from_numpy(np.ascontiguousarray(narrow)).cuda()))
            off += L
        assert off >= len(rows)
        out[name] = (rows, cuts)
    assert (out["u16"][0].sum(1) == 262140).any() and (out["u32"][0].sum(1) == 4 * ((1 << 30) - 1)).any()
    return out


def _codes(oracle, rows, alphas, keep, thr, min_cov, band):
    """the oracle's 4-bit mask of every row (bit 0 = A), coverage rules applied"""
    return _CODE_OF[_reference_sequence(oracle, rows.astype(np.float64), alphas, keep, thr, min_cov, band)]


def _pack(mask):
    out = np.zeros((len(mask) + 1) // 2, np.uint8)
    out |= mask[0::2]
    out[:len(mask) // 2] |= mask[1::2] << 4
    return out


def _exact(oracle, rows, alphas):
    """the exact posterior (threshold 0) of one cell per total class of `rows`: the second-largest distinct value of the class's richest
    row, or its only one -> ({total: posterior}, the posteriors of every row)"""
    post = oracle.calculate_posteriors(rows.astype(np.float64), alphas, False, 0.0)
    rs = rows.sum(1)
    exact = {}
    for t in sorted(set(rs.tolist())):
        cls = np.where(rs == t)[0]
        r = cls[np.argmax([len(set(rows[i].tolist())) for i in cls])]
        vals = np.unique(post[r])[::-1]
        vals = vals[vals > 0] if (vals > 0).any() else vals
        exact[t] = float(vals[min(1, len(vals) - 1)])
    return exact, post


def _on_both_sides(rows, post, exact):
    """the chosen thresholds really are posteriors of cells of `rows`, at every total class either side of the table's edge"""
    rs = rows.sum(1)
    for t, v in exact.items():
        assert (post[rs == t] == v).any(), t
    assert sum(t < 4096 for t in exact) >= 4 and sum(t >= 4096 for t in exact) >= 4


@pytest.mark.parametrize("aname", sorted(ALPHAS))
def test_codes_at_the_route_edges(aname, dev, oracle, tables, torch_mod):
    alphas = ALPHAS[aname]
    # thresholds: a cell of every total class of the uint16 table (its rows take the SHIFT = 4 screen above 4095; at 262 140 the only
    # row it can hold is four times 65 535) and of the uint32 table, the doubles either side of each, 0.01 and 0.3
    exact16, post16 = _exact(oracle, tables["u16"][0], alphas)
    exact32, post32 = _exact(oracle, tables["u32"][0], alphas)
    _on_both_sides(tables["u16"][0], post16, exact16)
    _on_both_sides(tables["u32"][0], post32, exact32)
    assert {4095, 4096, 4097, 65535, 262140} <= set(exact16) and {4095, 4096, 4097, (1 << 24) - 1, (1 << 24) + 1} <= set(exact32)
    thrs = {0.01, 0.3}
    for v in list(exact16.values()) + list(exact32.values()):
        thrs |= {v, float(np.nextafter(v, 0.0)), float(np.nextafter(v, 1.0))}
    thrs = sorted(thrs)
    assert len(thrs) >= 3 * 8 + 2
    every_rule = (0.01, 0.3, exact16[4096], exact16[262140])
    calls = 0
    for n, (thr, keep) in enumerate(itertools.product(thrs, (False, True))):
        # every threshold and keep value with one coverage rule, the rules taken in turn; four thresholds with every rule; always
        # every window of both tables
        rules = RULES if thr in every_rule else [RULES[n % len(RULES)]]
        for min_cov, band in rules:
            for name in ("u16", "u32"):
                rows, cuts = tables[name]
                want = _codes(oracle, rows, alphas, keep, thr, min_cov, band)
                for idx, L, counts in cuts:
                    got = dev.posterior_codes_device(counts, alphas, keep, thr, min_cov=min_cov, cov_band=band).cpu().numpy()
                    exp = _pack(want[idx])
                    calls += 1
                    if not np.array_equal(got, exp):
                        b = int(np.where(got != exp)[0][0])
                        raise AssertionError((aname, name, L, thr, keep, min_cov, band, "byte", b, int(got[b]), int(exp[b]),
                                              rows[idx[2 * b:2 * b + 2]].tolist()))
    print("%s: %d thresholds, %d calls" % (aname, len(thrs), calls))


def test_rules_mask_what_the_reference_masks(oracle, tables):
    """the expected masks themselves: each band and min_cov of the list masks exactly the totals it names"""
    rows = tables["u32"][0]
    rs = rows.sum(1)
    a = ALPHAS["cli"]
    plain = _codes(oracle, rows, a, False, 0.3, 0, None)
    for band, inside in (((2.0, 4.0), (rs >= 2) & (rs <= 4)), ((2.5, 2.7), rs < 0), ((4095.5, 4096.5), rs == 4096), ((-3.0, 0.5), rs == 0),
                         ((-3.0, -1.0), rs < 0)):
        got = _codes(oracle, rows, a, False, 0.3, 0, band)
        assert (got[inside] == 15).all() and np.array_equal(got[~inside], plain[~inside]), band
    for mc in MIN_COVS:
        got = _codes(oracle, rows, a, False, 0.3, mc, None)
        assert (got[rs < mc] == 15).all() and np.array_equal(got[rs >= mc], plain[rs >= mc])
    assert (plain[rs == 4096] != 15).any() and (plain[rs == 4095] != 15).any()


def _profile(hiplib, torch, counts, nbins, wide):
    from tracs_amd import device as dev
    L = counts.shape[0]
    c = torch.from_numpy(np.ascontiguousarray(counts, np.float64)).cuda()
    hist = torch.full((nbins,), -1, dtype=torch.int64, device="cuda")
    narrow = torch.full((max(L, 1), 4), -1, dtype=torch.int32 if wide else torch.int16, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    fn = hiplib.tracs_coverage_profile_device32 if wide else hiplib.tracs_coverage_profile_device
    rc = fn(dev._ptr(c), L, dev._ptr(hist), nbins, dev._ptr(narrow), dev._ptr(bad), dev._stream())
    assert rc == 0, hiplib.tracs_last_error()
    torch.cuda.synchronize()
    n = narrow.cpu().numpy()
    return hist.cpu().numpy(), (n.view(np.uint32) if wide else n.view(np.uint16)).astype(np.int64), int(bad.item())


@pytest.mark.parametrize("wide", (False, True), ids=("u16", "u32"))
def test_coverage_profile(wide, hiplib, torch_mod):
    """the histogram's LDS bins (totals below 8192), its global tail, the clamp to the last bin, the narrowed counts and the `bad` flag"""
    from tracs_amd.align_post import COV_BINS
    cap = (1 << 30) - 1 if wide else 65535
    for nbins in (COV_BINS, 100):
        for L in (1000, 70001):
            rng = np.random.default_rng(L + nbins)
            counts = rng.poisson(9.0, (L, 4)).astype(np.int64)
            deep = rng.random(L) < 0.2
            counts[deep] = rng.integers(0, min(cap, 70000) + 1, (int(deep.sum()), 4))
            special = [0, 1, 8191, 8192, 8193, nbins - 2, nbins - 1, nbins, nbins + 5000, 4 * cap]
            for j, t in enumerate(special):
                t = min(t, 4 * cap)
                q = [min(cap, t - t // 2), 0, 0, 0]                         # t split over the alleles within the cap
                rest = t - q[0]
                for k in (1, 2, 3):
                    q[k] = min(cap, rest)
                    rest -= q[k]
                assert rest == 0
                counts[37 * j + 3] = np.roll(q, j)
                counts[L - 1 - 41 * j] = np.roll(q, j + 1)
            rs = counts.sum(1)
            hist, narrow, bad = _profile(hiplib, torch_mod, counts, nbins, wide)
            want = np.bincount(np.minimum(rs, nbins - 1), minlength=nbins)
            assert bad == 0 and np.array_equal(narrow, counts), (nbins, L)
            assert np.array_equal(hist, want), (nbins, L, np.where(hist != want)[0][:5])
            assert want[nbins - 1] >= 2 and hist.sum() == L
    base = np.full((1000, 4), 3.0)
    for value, narrow_bad, wide_bad in ((65535.0, 0, 0), (65536.0, 1, 0), (2.0 ** 30 - 1, 1, 0), (2.0 ** 30, 1, 1), (2.5, 1, 1), (-1.0, 1, 1),
                                        (np.nan, 1, 1), (np.inf, 1, 1)):
        x = base.copy()
        x[617, 2] = value
        assert _profile(hiplib, torch_mod, x, 100, wide)[2] == (wide_bad if wide else narrow_bad), value
    hist, _, bad = _profile(hiplib, torch_mod, np.zeros((0, 4)), 100, wide)      # no site: an empty histogram
    assert bad == 0 and not hist.any()


def test_consensus_codes(hiplib, tables, torch_mod):
    """--consensus: the first allele with the largest count, every allele below min_cov, on the row table (ties in every allele order)"""
    from tracs_amd import device as dev
    torch = torch_mod
    for name in ("u16", "u32"):
        rows, cuts = tables[name]
        fn = hiplib.tracs_consensus_codes_device if name == "u16" else hiplib.tracs_consensus_codes_device32
        for min_cov in MIN_COVS:
            want = (1 << np.argmax(rows, axis=1)).astype(np.uint8)
            want[rows.sum(1) < min_cov] = 15
            for idx, L, counts in cuts:
                codes = torch.full(((L + 1) // 2,), 0xEE, dtype=torch.uint8, device="cuda")
                assert fn(dev._ptr(counts), L, min_cov, dev._ptr(codes), dev._stream()) == 0, hiplib.tracs_last_error()
                assert np.array_equal(codes.cpu().numpy(), _pack(want[idx])), (name, min_cov, L)
