"""The prior fit (csrc/dirichlet.hip) against tests/golden/dirichlet_hp_golden.json: alphas and iteration counts from the definition
at 50 digits (tests/hp_dirichlet.py), and the fit's digamma against its true values on a grid.  Nothing here is evaluated in high
precision; the fixture is read.

Every case's kept rows are laid among monomorphic and empty sites, the alleles of each row shuffled with a fixed seed (the kernel
sorts them).  Required: iters_out equal to the fixture's; every alpha within max(32 x the oracle's own recorded error on that case,
64 ulp) of the 50-digit value -- the device sums in another order with another digamma, a second draw of the error the oracle's f64
evaluation shows, amplified by the same contraction of the iteration; a row lost or doubled moves the alphas by about 1 / M >= 1e-4 and
an iteration more or less by about the last step -- and alphas the definition makes exactly 0 or exactly 1e-16 exactly that.

digamma_pos, measured on an MI355X over the 3 576 grid points in units of ulp(max(|psi|, 1)): worst 5.80 at x = 0.6257 (3.54 on
[1e-16, 1], 5.80 on [0.01, 12], 1.38 on [10, 3e9], 2.69 on the half-integers, 1.98 at x = 1); scipy's psi on the same grid: 1.89, so
the bound is 15.1.  Before the recurrence was carried to x >= 10 (it stopped at 6, leaving the series' 1.6e-13 truncation) the same
measure, on the same GPU, was 598 at x = 1 (154 on [1e-16, 1], 597 on [0.01, 12], 1.38 on [10, 3e9], 171 on the half-integers).

Measured on an MI355X, per case: iterations (equal to the fixture's on every case), the worst relative error of an alpha against the
50-digit value, and the oracle's recorded error on the same case (CPU):

    d8_FPI_1e-05         1000  1.42e-13  1.4e-13
    d8_FPI_1e-11         1000  1.42e-13  1.4e-13
    d8_LOO_1e-05         1000  4.19e-15  5.1e-14
    d8_LOO_1e-11         1000  4.19e-15  5.1e-14
    d25_FPI_1e-05         596  2.62e-15  2.87e-14
    d25_FPI_1e-11        1000  2.08e-15  1.64e-14
    d25_LOO_1e-05         450  1.24e-15  8.82e-15
    d25_LOO_1e-11        1000  1.86e-15  1.06e-14
    d200_FPI_1e-05        763  3.42e-16  1.66e-15
    d200_FPI_1e-11       1000  4.73e-16  1.78e-15
    d200_LOO_1e-05       1000  1.42e-16  1.75e-14
    d200_LOO_1e-11       1000  1.42e-16  1.75e-14
    c60k                 1000  1.87e-16  7.24e-15
    c3e8                 1000  1.92e-15  8.07e-15
    k2                   1000  8.93e-14  1.01e-13
    k3                   1000  1.54e-13  1.5e-13
    k5                   1000  3.42e-13  3.39e-13
    k8                   1000  5.94e-13  8.47e-13
    two_converged         657  1.38e-15  1.67e-14
    two_max_iter           40  3.24e-15  5.34e-15
    d25_max_iter_0          0  7.47e-17  7.47e-17
    d25_max_iter_1          1  7.11e-16  3.1e-15
    d25_max_iter_31        31  1.78e-15  2.67e-14
    d25_max_iter_32        32  2.52e-15  2.85e-14
    d25_max_iter_33        33  2.46e-15  2.84e-14
    d25_max_iter_64        64  6.13e-16  1.26e-14
    d25_max_iter_65        65  7.95e-16  1.41e-14
    cut5                    0  0         0
    cut6                  536  1.21e-15  1.53e-15
    base_filter_0.05      611  7.71e-16  1.73e-15
    keep19_filter_0.05    680  8.02e-15  3.13e-14
    drop39_filter_0.05    611  7.71e-16  1.73e-15
    zero_filter_0.05      611  7.71e-16  1.73e-15

Run time of every new GPU test on an MI355X, call phase, in a run of the whole suite (this module's 37 tests and the 8 of
tests/test_gpu_posterior_routes.py; run alone the two modules take 3.95 s together, 1.4 s of it the first test's set-up of library and
runtime, and test_digamma_on_the_grid 0.15 s with the first kernel's load):
    test_codes_at_the_route_edges [cli] 0.18 s, [small_last] 0.18, [degenerate] 0.18, [equal] 0.13; test_coverage_profile [u16] 0.03,
    [u32] 0.03; test_rules_mask_what_the_reference_masks and test_consensus_codes below 0.005
    test_layouts_give_the_same_bits 0.12; test_degenerate_answers 0.05; test_no_stale_workspace 0.05; test_digamma_on_the_grid
    below 0.005
    test_fit_against_the_definition: k8 0.05; d25_FPI_1e-05, keep19_filter_0.05 0.04; two_converged, d25_FPI_1e-11, d200_FPI_1e-11,
    d200_FPI_1e-05, d8_LOO_1e-11, d8_FPI_1e-11, d8_FPI_1e-05, c60k, c3e8, k5, k3 0.03; k2, d25_LOO_1e-11, d8_LOO_1e-05,
    d200_LOO_1e-11, d200_LOO_1e-05, base_filter_0.05, drop39_filter_0.05, zero_filter_0.05, cut6 0.02; d25_LOO_1e-05, d25_max_iter_33,
    cut5 0.01; the other max_iter cases and two_max_iter below 0.005

Mutations, each built and run once against this module and then reverted:
  * the 1 / 132 term removed from digamma_pos: test_digamma_on_the_grid fails (worst 3 410 ulp, at x = 1), and so do 14 cases of
    test_fit_against_the_definition (of the 25 FPI ones; errors near 5e-12 against 5e-14 allowed on the 6-row table),
    test_layouts_give_the_same_bits, test_no_stale_workspace and test_degenerate_answers; the LOO cases pass, as they must.
  * `M <= 5` turned into `M < 5`: test_fit_against_the_definition[cut5] and test_degenerate_answers fail (5 kept rows are fitted:
    558 iterations instead of the degenerate answer); cut6 passes.

Layouts: L = 257 (two blocks, the second with one site) cannot hold the 791 kept rows of the depth-25 table, so that layout runs the
6-row table (and so does 65 536), and the depth-25 table runs at 1 025 (five blocks, the last with one site), 65 536 and
262 145 (the smallest L where a block's chunk is 512 and the last block is partial)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

import hp_dirichlet as H  # noqa: E402  (no mpmath needed for what is used here)

FIXTURE = os.path.join(HERE, "golden", "dirichlet_hp_golden.json")
with open(FIXTURE) as _fh:
    FX = json.load(_fh)
CASES = {c["name"]: c for c in FX["cases"]}
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def torch_mod(hiplib):
    import torch
    assert torch.cuda.is_available()
    return torch


def _sites(table, L, seed=1, forced=()):
    """float64 [L][K]: the table's rows, in its order, on sorted sites (the `forced` ones among them), each row's alleles shuffled;
    every other site monomorphic or empty.  The shuffle depends on the seed alone, so two layouts of a table differ only in where the
    rows lie."""
    rows = H.expand(table)
    M, K = rows.shape
    assert M <= L
    rows = np.take_along_axis(rows, np.random.default_rng(seed).permuted(np.tile(np.arange(K), (M, 1)), axis=1), 1)
    rng = np.random.default_rng(seed + 1000)
    out = np.zeros((L, K))
    mono = rng.random(L) < 0.7
    out[np.arange(L)[mono], rng.integers(0, K, L)[mono]] = rng.integers(1, 90, L)[mono]
    forced = sorted(set(int(f) for f in forced))
    free = np.setdiff1d(np.arange(L), forced)
    pos = np.sort(np.concatenate([np.array(forced, np.int64), rng.choice(free, M - len(forced), replace=False)])) if M > len(forced) \
        else np.array(forced[:M], np.int64)
    out[pos] = rows
    return np.ascontiguousarray(out)


def _fit(hiplib, counts, case, K=None):
    counts = np.ascontiguousarray(counts, np.float64)
    K = counts.shape[1] if K is None else K
    out, iters = np.full(K, np.nan), C.c_int(-1)
    filt = case["error_filt_threshold"]
    rc = hiplib.tracs_find_dirichlet_priors(counts.ctypes.data_as(DP), counts.shape[0], K, case["max_iter"], case["tol"],
                                            1 if case["method"] == "LOO" else 0, -1.0 if filt is None else filt, out.ctypes.data_as(DP),
                                            C.byref(iters))
    assert rc == 0, hiplib.tracs_last_error()
    return out, iters.value


def _fit_device(hiplib, torch, counts, case):
    """the device entry point on a stream of its own"""
    from tracs_amd import device as dev
    t = torch.from_numpy(np.ascontiguousarray(counts, np.float64)).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    out, iters = np.full(counts.shape[1], np.nan), C.c_int(-1)
    filt = case["error_filt_threshold"]
    rc = hiplib.tracs_find_dirichlet_priors_device(dev._ptr(t), counts.shape[0], counts.shape[1], case["max_iter"], case["tol"],
                                                   1 if case["method"] == "LOO" else 0, -1.0 if filt is None else filt,
                                                   out.ctypes.data_as(DP), C.byref(iters), C.c_void_p(stream.cuda_stream))
    assert rc == 0, hiplib.tracs_last_error()
    stream.synchronize()
    return out, iters.value


def _check(case, got, iters):
    hi, lo = np.array(case["alphas"]).T
    err = H.rel_errors(got, hi, lo)
    tol = np.maximum(32 * case["oracle_rel_err"], 64 * np.spacing(np.abs(hi)) / np.where(hi == 0, 1.0, np.abs(hi)))
    print("%-22s iterations %4d (fixture %4d)  worst alpha error %.3g  (oracle's %.3g, allowed %.3g)"
          % (case["name"], iters, case["iters"], err.max(), case["oracle_rel_err"], tol.min()))
    assert iters == case["iters"], (case["name"], iters, case["iters"])
    exact = (hi == 0.0) | ((hi == H.CLAMP) & (lo == 0.0)) | (case["kept_rows"] <= 5)
    assert np.array_equal(got[exact], hi[exact]), (case["name"], got, hi)
    assert (err[~exact] <= tol[~exact]).all(), (case["name"], err, tol)
    return float(err.max())


def _length(case):
    return 3 * int(sum(r[-1] for r in H.case_table(FX, case))) + 7


def test_digamma_on_the_grid(hiplib, torch_mod):
    """digamma_pos on the 3 576 grid points: worst error <= 8 x scipy's worst on the same grid (the device's log and divides, up to ten
    recurrence terms; a truncated series or a wrong coefficient shows as hundreds of ulp), and two evaluations agree bit for bit.
    Measured worst: 5.80 ulp at x = 0.6257 (the module's docstring has the figure per part of the grid)."""
    xs = H.digamma_grid()
    g = FX["digamma"]
    assert len(xs) == g["points"] and [xs[0], xs[-1]] == g["x_first_last"] and float(np.sum(xs)) == g["x_sum"]
    out = [np.full(len(xs), np.nan) for _ in range(2)]
    for o in out:
        assert hiplib.tracs_debug_digamma(xs.ctypes.data_as(DP), len(xs), o.ctypes.data_as(DP)) == 0, hiplib.tracs_last_error()
    assert np.array_equal(out[0] - out[1], np.zeros(len(xs))) and np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64))
    err = np.abs(H.ulp_errors(out[0], FX["digamma_hi"], H.digamma_lo(FX["digamma_hi"], FX["digamma_lo_ulp"])))
    w = int(np.argmax(err))
    bound = 8 * g["scipy_worst_ulp"]
    print("digamma_pos: worst %.3g ulp at x = %r (psi = %r); at x = 1: %.3g ulp; scipy's worst %.3g ulp; bound %.3g"
          % (err[w], float(xs[w]), FX["digamma_hi"][w], err[int(np.where(xs == 1.0)[0][0])], g["scipy_worst_ulp"], bound))
    for name, sl in (("[1e-16, 1]", slice(0, 300)), ("[0.01, 12]", slice(300, 3300)), ("[10, 3e9]", slice(3300, 3500)),
                     ("half-integers", slice(3500, 3570)), ("1, 2, 6, 10, root", slice(3570, 3576))):
        print("    %-18s worst %.3g ulp" % (name, err[sl].max()))
    assert err.max() <= bound, (err[w], float(xs[w]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_against_the_definition(name, hiplib, torch_mod):
    case = CASES[name]
    counts = _sites(H.case_table(FX, case), _length(case))
    got, iters = _fit(hiplib, counts, case)
    _check(case, got, iters)
    again, iters2 = _fit(hiplib, counts, case)                                   # the same call twice: the same bits
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64)) and iters2 == iters
    if name in ("d25_FPI_1e-05", "d8_LOO_1e-11", "k8", "two_converged", "keep19_filter_0.05", "cut5", "d25_max_iter_33"):
        dgot, diters = _fit_device(hiplib, torch_mod, counts, case)              # the device entry point, a stream of its own
        assert np.array_equal(got.view(np.uint64), dgot.view(np.uint64)) and diters == iters


def test_layouts_give_the_same_bits(hiplib, torch_mod):
    """Where the kept rows lie does not matter: the compaction keeps them in site order across block boundaries (sites 0, 255, 256,
    chunk - 1, chunk, L - 1 hold rows), so alphas and iteration count are bit-identical between layouts, and right."""
    case, table = CASES["d25_FPI_1e-05"], FX["tables"]["d25"]
    seen = []
    for L, forced in ((1025, (0, 255, 256, 1024)), (65536, (0, 255, 256, 65535)), (262145, (0, 255, 256, 511, 512, 262144))):
        counts = _sites(table, L, forced=forced)
        kept = H.select_rows(counts, case["error_filt_threshold"])
        assert len(kept) == case["kept_rows"] and all(np.count_nonzero(counts[f]) > 1 for f in forced)
        got, iters = _fit(hiplib, counts, case)
        _check(case, got, iters)
        seen.append((got.view(np.uint64).tolist(), iters))
    assert seen[0] == seen[1] == seen[2]
    small, few = CASES["cut6"], FX["tables"]["cut6"]                              # two blocks, the second with one site
    a = _fit(hiplib, _sites(few, 257, forced=(0, 255, 256)), small)
    b = _fit(hiplib, _sites(few, 65536, forced=(0, 255, 256, 65535)), small)
    _check(small, *a)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and a[1] == b[1]
    # many rows in two blocks: the first distinct rows of the depth-25 table, about 200 kept rows, at 257 sites and at 65 536 (no
    # 50-digit value for this cut: the bits agree, and the oracle's fit of the same rows is within 2e-12, twice the 32 x 2.9e-14
    # either is allowed against the definition on the whole table)
    part, n = [], 0
    for r in table:
        if n + r[-1] > 200:
            break
        part.append(r)
        n += r[-1]
    assert 150 <= n <= 200
    a = _fit(hiplib, _sites(part, 257, forced=(0, 255, 256)), case)
    b = _fit(hiplib, _sites(part, 65536, forced=(0, 255, 256, 65535)), case)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and a[1] == b[1] > 0
    from oracle import oracle as O
    want, it = O.find_dirichlet_priors(H.expand(part), error_filt_threshold=case["error_filt_threshold"], return_iters=True)
    assert it == a[1] and np.allclose(a[0], want, rtol=2e-12, atol=0)


def test_no_stale_workspace(hiplib, torch_mod):
    """the largest table (8 MB, 1000 iterations), then a 40-site table, then the largest again: the same bits both times"""
    big_case, small_case = CASES["d25_FPI_1e-11"], CASES["cut6"]
    big = _sites(FX["tables"]["d25"], 262145)
    small = _sites(FX["tables"]["cut6"], 40)
    first = _fit(hiplib, big, big_case)
    mid = _fit(hiplib, small, small_case)
    second = _fit(hiplib, big, big_case)
    _check(big_case, *first)
    _check(small_case, *mid)
    assert np.array_equal(first[0].view(np.uint64), second[0].view(np.uint64)) and first[1] == second[1] == 1000


def test_degenerate_answers(hiplib, torch_mod):
    """5 kept rows: (0, .., 0, 1) without an iteration, 6: a fit (also in the parametrised cases); K = 1 -> [1.0]; no site at all -> the
    degenerate answer; the filter's equality rows are kept, its dropped rows leave the base table's alphas"""
    for name in ("cut5", "cut6"):
        got, iters = _fit(hiplib, _sites(FX["tables"][name], 300), CASES[name])
        _check(CASES[name], got, iters)
        assert (iters == 0) == (name == "cut5")
    assert CASES["cut5"]["alphas"] == [[0.0, 0.0]] * 3 + [[1.0, 0.0]]
    plain = dict(max_iter=1000, tol=1e-5, method="FPI", error_filt_threshold=None)
    got, iters = _fit(hiplib, np.arange(1.0, 51.0).reshape(50, 1), plain)
    assert got.tolist() == [1.0] and iters == 0
    got, iters = _fit(hiplib, np.zeros((1, 4)), plain)                           # one empty site
    assert got.tolist() == [0.0, 0.0, 0.0, 1.0] and iters == 0
    out, it = np.full(4, np.nan), C.c_int(-1)                                    # L = 0
    assert hiplib.tracs_find_dirichlet_priors(np.zeros(4).ctypes.data_as(DP), 0, 4, 1000, 1e-5, 0, 0.01, out.ctypes.data_as(DP), C.byref(it)) == 0
    assert out.tolist() == [0.0, 0.0, 0.0, 1.0] and it.value == 0
    res = {}
    for name in ("base", "keep19", "drop39", "zero"):
        case = CASES[name + "_filter_0.05"]
        counts = _sites(H.case_table(FX, case), _length(case))
        assert len(H.select_rows(counts, 0.05)) == case["kept_rows"]
        res[name] = _fit(hiplib, counts, case)
        _check(case, *res[name])
    assert abs(res["keep19"][0][0] - res["base"][0][0]) > 0.1                    # the 400 equality rows were in the fit
