"""The checks of tests/test_pairsnp_ref.py, run as a child process: `python tests/pairsnp_ref_check.py SECTION`.

A process of its own because the live comparison loads oracle/_ref/_tracs_ref_pairsnp, built with the reference's -ffast-math, and
loading such a library switches the whole process to flush-to-zero arithmetic (as tests/test_oracle_vs_ref.py explains).  Every
section compares against tests/golden/pairsnp_ref_golden.npz ("stored") and, where oracle/_ref is present, against the module
itself ("live": both builds, which must also reproduce the stored values).  Prints "OK SECTION stored[+live] ..." on success.

The reference's filter walks the whole bitset once per SNP (range_count starts at find_first), so a list of d SNPs costs d^2 / 2
steps: minutes for the four hp cases with d >= 65 536.  Those are compared live by the generator only; here, stored."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import pairsnp_ref_cases as PC  # noqa: E402
from oracle import oracle as O  # noqa: E402

LIVE_MAX_D = 9000


def _modules():
    mods = [m for m in (O.ref_pairsnp_module(strict=True), O.ref_pairsnp_module()) if m is not None]
    assert len(mods) in (0, 2), "one build of oracle/_ref/_tracs_ref_pairsnp is missing"
    return mods


def _same(got, want, what):
    assert len(got) == len(want), (what, "lengths", len(got), len(want))
    for name, g, w in zip(("rows", "cols", "d", "nn", "filt"), got, want):
        g, w = np.asarray(g, np.int64), np.asarray(w, np.int64)
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, g.shape, w.shape, np.nonzero(g != w)[0][:8] if g.shape == w.shape else None)


def pairloop():
    """O.pairsnp from FASTA, O.pairsnp_arrays, O.brute_pairsnp and O.filter_recomb_pairs = the reference, exactly, on every case"""
    meta, arrays = PC.load()
    mods = _modules()
    pairs = 0
    for case in meta["cases"] + meta["filter_cases"]:
        seqs = arrays["aln/" + case["aln"]]
        want = PC.expected(arrays, case)
        name = case["name"]
        with tempfile.TemporaryDirectory() as td:
            fastas = PC.write_fastas(case, seqs, td)
            for m in mods:                                           # the live reference reproduces what is stored
                out = m.ref_pairsnp(fastas, 1, case["dist"], case["filter"])
                _same((out[0], out[1], out[2], out[5], out[4]), want, (name, "live reference != stored"))
                assert out[3] == PC.names_of(seqs.shape[0]), name
            out = O.pairsnp(fastas, 1, case["dist"], case["filter"])
        _same((out[0], out[1], out[2], out[5], out[4]), want, (name, "O.pairsnp"))
        assert out[3] == PC.names_of(seqs.shape[0]), name
        _same(O.pairsnp_arrays(seqs, n0=case["n0"], dist=case["dist"]), want[:4], (name, "O.pairsnp_arrays"))
        _same(O.brute_pairsnp(seqs, n0=case["n0"], dist=case["dist"]), want[:4], (name, "O.brute_pairsnp"))
        if case["filter"]:
            filt = O.filter_recomb_pairs(seqs, want[0].astype(np.uint64), want[1].astype(np.uint64))
            _same((filt,), (want[4],), (name, "O.filter_recomb_pairs"))
            assert (want[4] < want[2]).any()
        else:
            assert not want[4].any() and len(want[4]) == len(want[2]), name
        pairs += len(want[0])
    print("OK pairloop stored%s: %d cases, %d pairs" % ("+live" if mods else "", len(meta["cases"]) + len(meta["filter_cases"]), pairs))


def _hp():
    import hp_filter as H
    with open(os.path.join(HERE, "golden", "filter_hp_golden.json")) as fh:
        hp_cases = json.load(fh)["cases"]
    return H, hp_cases, PC.hp_lists(H, hp_cases)


def positions():
    """O.filter_recomb_positions = ref_filter_recomb_positions = hp_filter.filter_positions on every list of filter_hp_golden.json"""
    meta, arrays = PC.load()
    H, hp_cases, lists = _hp()
    ref = arrays["hp/ref"].reshape(-1)
    assert len(lists) == len(ref) == meta["hp_lists"] == 3 * len(hp_cases)
    mods = _modules()
    live = fresh = 0
    for t, (L, d, pos) in enumerate(lists):
        assert len(pos) == d
        assert O.filter_recomb_positions(pos, L) == ref[t], ("oracle != reference", L, d, t % 3)
        c = hp_cases[t // 3]                                        # what hp_filter.filter_positions returned when the hp fixture was made
        assert ref[t] == (c["expected"], c["probe"][1], c["probe"][2])[t % 3], ("reference != definition (stored)", L, d, t % 3)
        if d <= LIVE_MAX_D:
            kept, _, ill, margin = H.filter_positions(pos, L)       # and evaluated afresh at 50 digits
            assert ill == 0 and margin > H.MARGIN and kept == ref[t], ("reference != definition", L, d, t % 3, kept, ill)
            fresh += 1
            for m in mods:
                assert m.ref_filter_recomb_positions(L, pos.tolist()) == ref[t], ("live reference != stored", L, d, t % 3)
                live += 1
    # d <= 1 leaves before any window is looked at
    assert O.filter_recomb_positions(np.zeros(0, np.int64), 100) == 0 and O.filter_recomb_positions(np.array([99]), 100) == 1
    for m in mods:
        assert m.ref_filter_recomb_positions(100, []) == 0 and m.ref_filter_recomb_positions(100, [99]) == 1
    print("OK positions stored%s: %d lists, %d evaluated afresh at %d digits, %d live calls" % ("+live" if mods else "", len(lists), fresh, H.DPS, live))


def cdf():
    """|(1 - ref_cached_binomial_cdf(n, p, k)) - tail(n, k, p)| <= 1e-9 * 0.05 / d on n*, n* - 1 of every hp row and on every window of
    the planted-import alignments"""
    meta, arrays = PC.load()
    H, hp_cases, _ = _hp()
    cells, value = arrays["cdf/cells"], arrays["cdf/value"]
    have = {tuple(c) for c in cells.tolist()}
    # the cells are the ones the issue names: recomputed from the fixtures, not taken on trust
    need = {(c["L"], c["d"], n - e, k) for c in hp_cases for k, n in enumerate(c["row"], start=2) if n is not None for e in (0, 1)}
    for case in meta["filter_cases"]:
        if case["dist"] != PC.INT_MAX:
            continue
        seqs = arrays["aln/" + case["aln"]]
        m = O._MASK[seqs]
        r, c = PC.expected(arrays, case)[:2]
        for i, j in zip(r.tolist(), c.tolist()):
            pos = np.nonzero((m[i] & m[j]) == 0)[0].astype(np.int64)
            L, d = seqs.shape[1], len(pos)
            if d <= 1:
                continue
            _, _, wh = H.window(L, d)
            lo = np.searchsorted(pos, np.maximum(0, pos - wh), "left")
            hi = np.searchsorted(pos, np.minimum(L, pos + wh + 1), "left")
            need |= {(L, d, int(n), int(k)) for k, n in zip(hi - lo, pos[hi - 1] - pos[lo] + 1) if k > 1}
    assert need == have and len(have) == meta["measured"]["cdf_cells"], (len(need), len(have))
    mods = _modules()
    worst = {"stored": 0.0, "live": 0.0}
    with H.mp.workdps(H.DPS):
        for (L, d, n, k), v in zip(cells.tolist(), value.tolist()):
            p, thr, _ = H.window(L, d)
            t = H.tail(n, k, p)
            bound = H.mpf(H.MARGIN) * H.mpf(thr)
            for src, x in [("stored", v)] + [("live", m.ref_cached_binomial_cdf(n, p, k)) for m in mods]:
                err = abs(H.mpf(1.0 - x) - t)
                assert err <= bound, (src, L, d, n, k, float(err / H.mpf(thr)))
                worst[src] = max(worst[src], float(err / H.mpf(thr)))
                assert (1.0 - x >= thr) == (t >= H.mpf(thr)), ("the stand-in decides a cell against the definition", src, L, d, n, k)
    if mods:
        assert mods[0].ref_cached_binomial_cdf(10, 0.3, 10) == 1.0 and mods[0].ref_cached_binomial_cdf(10, 0.0, 3) == 1.0
    print("OK cdf stored%s: %d cells, largest |error| / thr stored %.3g live %.3g (bound %.0e)"
          % ("+live" if mods else "", len(cells), worst["stored"], worst["live"], H.MARGIN))
    assert worst["stored"] <= 2 * meta["measured"]["standin_max_error_over_threshold"]


def range_count():
    """the reference's range_count = (last - first + 1, count) of the set sites within [start, end): live only"""
    mods = _modules()
    rng = np.random.default_rng(3)
    n = 0
    for m in mods:
        for L in (1, 64, 65, 1000):
            for _ in range(20):
                pos = np.sort(rng.choice(L, size=int(rng.integers(1, min(L, 40) + 1)), replace=False))
                for _ in range(10):
                    a, b = sorted(rng.integers(0, L + 1, 2).tolist())
                    inside = pos[(pos >= a) & (pos < b)]
                    want = (int(inside[-1] - inside[0] + 1), len(inside)) if len(inside) else (0, 0)
                    assert tuple(m.ref_range_count(L, pos.tolist(), a, b)) == want, (L, pos, a, b)
                    n += 1
    print("OK range_count %s: %d ranges" % ("live" if mods else "skipped (oracle/_ref absent)", n))


if __name__ == "__main__":
    {"pairloop": pairloop, "positions": positions, "cdf": cdf, "range_count": range_count}[sys.argv[1]]()
