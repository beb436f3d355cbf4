"""Every route of the recombination filter on pairs whose windows sit on the keep / drop boundary, against
tests/golden/filter_hp_golden.json: the filtered distances the definition gives at 50 digits (tests/hp_filter.py) for the crafted
sites of hp_filter.boundary_positions -- clusters of k SNPs spanning exactly n*(k) and n*(k) - 1 sites, the smallest surviving span
and one less, for every k the pair's d can hold -- and for two probes per (L, d) that tell the half window wh from wh + 1.  No case
has a cell within 1e-9 of the threshold (relative), so the comparison is exact.

One alignment per L: sample 0 is all A, and every other sample differs from it at the sites of one (L, d) case or probe; the pairs
are (0, s).  Nothing is evaluated in high precision here: the fixture holds the rows and the expected counts.

Mutation check (by hand, not part of the suite): `out = (unsigned)lo + (k == 5)` in flt_table_kernel makes
test_boundary_pairs_on_every_route[lists] fail and leaves [lists_no_table] passing."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

from test_filter_recomb import ROUTES  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "filter_hp_golden.json")
# the plane scan with a pair per lane in one batch too (ROUTES has it in batches): both extraction kernels on both
ALL_ROUTES = dict(ROUTES, scan_lanes={"TRACS_FILTER_LISTS": "0", "TRACS_FILTER_LANES_MIN": "0"})
_CACHE = {}


def _cases():
    if "fx" not in _CACHE:
        with open(FIXTURE) as fh:
            _CACHE["fx"] = json.load(fh)["cases"]
    return _CACHE["fx"]


def _lengths():
    return sorted({c["L"] for c in _cases()})


def _sites(L):
    """[(d, sorted sites, expected filtered distance)] of the samples 1, 2, .. of the alignment of length L"""
    if ("sites", L) not in _CACHE:
        import hp_filter as H
        out = []
        for c in _cases():
            if c["L"] != L:
                continue
            d = c["d"]
            out.append((d, np.asarray(H.boundary_positions(L, d, c["row"]), np.int64), c["expected"]))
            shape, at_wh, beyond = c["probe"]
            out.append((d, np.asarray(H.probe_positions(L, d, shape, c["wh"]), np.int64), at_wh))
            out.append((d, np.asarray(H.probe_positions(L, d, shape, c["wh"] + 1), np.int64), beyond))
        _CACHE["sites", L] = out
    return _CACHE["sites", L]


def _alignment(L):
    if ("aln", L) not in _CACHE:
        sites = _sites(L)
        seqs = np.full((1 + len(sites), L), ord("A"), np.uint8)
        for s, (d, pos, _) in enumerate(sites, start=1):
            assert len(pos) == d
            seqs[s, pos] = ord("C")
        seqs.setflags(write=False)
        _CACHE["aln", L] = seqs
    return _CACHE["aln", L]


def _decorated(L):
    """the same SNP sites under things that must not change them: N and a compatible partial code in sample s next to its SNPs
    (inside the clusters' spans), N in sample 0 at sites where no sample has a SNP, lower case, three substitution letters"""
    sites = _sites(L)
    seqs = np.full((1 + len(sites), L), ord("A"), np.uint8)
    taken = np.zeros(L + 3, bool)
    for s, (d, pos, _) in enumerate(sites, start=1):
        snp = np.zeros(L + 3, bool)
        snp[pos] = True
        taken |= snp
        seqs[s, pos] = np.frombuffer(b"CGT", np.uint8)[pos % 3]
        low = pos[::2]
        seqs[s, low] |= 0x20                                       # lower case
        nxt = pos[:-1][~snp[pos[:-1] + 1]] + 1                     # the site after a SNP, where that is no SNP: between two of a cluster
        seqs[s, nxt[::6]] = ord("N")
        seqs[s, nxt[1::6]] = ord("R")                              # A or G: compatible with sample 0's A
        seqs[s, nxt[2::12]] = ord("n")
    free = np.nonzero(~taken[:L])[0]
    seqs[0, free[::101]] = ord("N")
    seqs[0, free[3::7]] = ord("a")
    return seqs


def _filter(dev, aln, samples, ds):
    import torch
    rows = torch.zeros(len(samples), dtype=torch.int32, device="cuda")
    cols = torch.from_numpy(np.asarray(samples, np.int32)).cuda()
    dd = torch.from_numpy(np.asarray(ds, np.int32)).cuda()
    return dev.filter_recomb_pairs(aln, rows, cols, dd).cpu().numpy()


def _check_alignment(dev, seqs, L, route, subset_first=True):
    sites = _sites(L)
    aln = dev.Alignment(seqs.shape[0], L)
    aln.pack(seqs)
    s = np.arange(1, len(sites) + 1)
    d = np.array([x[0] for x in sites])
    want = np.array([x[2] for x in sites], np.int32)
    # a subset first (the threshold rows are built per call from the d that call marks), then all in reverse, then all
    orders = ([np.arange(len(s))[1::2]] if subset_first else []) + [np.arange(len(s))[::-1], np.arange(len(s))]
    for o in orders:
        got = _filter(dev, aln, s[o], d[o])
        bad = np.nonzero(got != want[o])[0]
        assert not len(bad), (route, L, [(int(d[o][i]), int((o[i]) % 3), int(got[i]), int(want[o][i])) for i in bad[:8]])
    info = dev.filter_index_info(aln)
    aln.close()
    return info


@pytest.mark.parametrize("route", sorted(ALL_ROUTES))
def test_boundary_pairs_on_every_route(hiplib, monkeypatch, route):
    """filter_recomb_pairs of the pairs (0, s) = the definition's filtered distance, exactly, on every route and for every L"""
    from tracs_amd import device as dev
    for k, v in ALL_ROUTES[route].items():
        monkeypatch.setenv(k, v)
    for L in _lengths():
        info = _check_alignment(dev, _alignment(L), L, route)
        assert info is not None and info["lists"] == (not route.startswith("scan")), (route, L, info)


@pytest.mark.parametrize("route", ["lists", "scan"])
def test_boundary_pairs_decorated(oracle, hiplib, monkeypatch, route):
    """N, compatible partial codes and lower case around the SNPs change neither the SNP sites nor the filtered distances"""
    from tracs_amd import device as dev
    for k, v in ALL_ROUTES[route].items():
        monkeypatch.setenv(k, v)
    for L in _lengths():
        seqs = _decorated(L)
        assert (seqs != _alignment(L)).mean() > 1e-4
        r, c, d, _ = oracle.pairsnp_arrays(seqs)
        first = r == 0
        assert np.array_equal(c[first], np.arange(1, seqs.shape[0])) and np.array_equal(d[first], [x[0] for x in _sites(L)])
        info = _check_alignment(dev, seqs, L, route, subset_first=False)
        assert info is not None and info["lists"] == (route == "lists"), (route, L, info)


def test_table_rows_are_rebuilt_per_alignment(hiplib):
    """the threshold rows depend on L: a handle of 120 000 sites filtered after one of 9 000 (both hold d = 2, and their other d
    lie in the same rows' range) gives its own answers, in either order"""
    from tracs_amd import device as dev
    for order in ((9000, 120000), (120000, 9000)):
        handles = []
        for L in order:
            seqs = _alignment(L)
            aln = dev.Alignment(seqs.shape[0], L)
            aln.pack(seqs)
            handles.append((L, aln))
            sites = _sites(L)
            got = _filter(dev, aln, np.arange(1, len(sites) + 1), [x[0] for x in sites])
            assert np.array_equal(got, [x[2] for x in sites]), (order, L)
        for L, aln in handles:                                   # and again, with both alive
            sites = _sites(L)
            got = _filter(dev, aln, np.arange(1, len(sites) + 1), [x[0] for x in sites])
            assert np.array_equal(got, [x[2] for x in sites]), (order, L)
            aln.close()


def test_boundary_pairs_end_to_end(hiplib, tmp_path):
    """FASTA -> pairsnp with the filter: the (0, s) rows carry the fixture's filtered distances"""
    from tracs_amd import api, synth
    L = 120000
    sites = _sites(L)
    fa = os.path.join(str(tmp_path), "boundary.fa")
    synth.write_fasta(fa, np.array(_alignment(L)), width=80)
    r, c, d, names, filt, nn = api.pairsnp_arrays([fa], 1, 2147483647, True)
    r, c, d, filt = (np.asarray(x).astype(np.int64) for x in (r, c, d, filt))
    first = r == 0
    assert np.array_equal(c[first], np.arange(1, len(sites) + 1))
    assert np.array_equal(d[first], [x[0] for x in sites])
    assert np.array_equal(filt[first], [x[2] for x in sites]), np.nonzero(filt[first] != [x[2] for x in sites])
    assert (filt <= d).all()
