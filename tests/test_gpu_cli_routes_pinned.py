"""Every route of `tracs distance` and `tracs pair-sites` end to end, without a rule and under all of them: the files written (sha256,
line count), the INFO messages in order and the [stage] names equal what the commit before the host layer moved onto
tracs_amd/handle.py wrote and logged (tests/golden/cli_routes_golden.json, written on the GPU by that commit's package:
tests/golden/make_cli_routes_golden.py).  The API half compares the four array entry points -- called with nothing, with `sites=`
alone and with the rule keywords -- to the oracle on the cut alignment and their `info` keys to the golden's."""
import json
import os

import numpy as np
import pytest

import cli_routes_common as T
from site_rules_common import is_n_table

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_routes_golden.json")))
_PLACEHOLDER = dict(td="", fa="", q="", db="", meta="", groups="", bed="", ref="", max_hosts=1)
ROUTE_NAMES = [r[0] for r in T.routes(_PLACEHOLDER, 1)]
CALL_NAMES = ["%s:%s" % (fn, how) for fn in ("pairsnp_arrays", "nearest_arrays", "distance_histogram", "pair_sites")
              for how in ("nothing", "sites", "rules")]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, hiplib, oracle):
    inp = T.make_inputs(str(tmp_path_factory.mktemp("cli_routes")))
    isn = inp["isn"] = is_n_table(hiplib)
    # from the data, before anything runs: --max-sample-n-share 0.5 drops exactly the two N-heavy samples, --max-n-share and
    # Sites(max_n_samples) each drop columns the files keep, -D and --min-sites each cut some pairs and not all
    samples, cols, counts, lp = T.ruled_alignment(inp, isn)
    assert np.flatnonzero(~samples).tolist() == list(T.HEAVY) and lp == T.L - 116
    assert 0 < cols.sum() < lp
    inp["min_sites"], inp["max_n"] = T.min_sites_of(inp, isn), T.max_n_of(inp, isn)
    assert inp["max_n"] >= 0 and (isn[inp["seqs"]].sum(axis=0)[inp["keep"]] > inp["max_n"]).any()
    r, c, d, nn = oracle.pairsnp_arrays(inp["seqs"][samples][:, cols])
    assert 0 < (d <= inp["dist"]).sum() < len(d)
    nn = nn[d <= inp["dist"]]
    assert (nn < inp["min_sites"]).any() and (nn >= inp["min_sites"]).any()
    return inp


@pytest.fixture(scope="module")
def runs(inputs):
    """every route once, in the order of the list (pair-sites reads the ruled run's output)"""
    return {r[0]: T.run_route(inputs, r) for r in T.routes(inputs, inputs["min_sites"])}


def test_the_golden_holds_the_routes():
    assert sorted(GOLDEN["routes"]) == sorted(ROUTE_NAMES) and sorted(GOLDEN["api_info_keys"]) == sorted(CALL_NAMES)
    assert GOLDEN["routes"]["staged"]["stages"] and all(not g["stages"] for n, g in GOLDEN["routes"].items() if n != "staged")
    for name, g in GOLDEN["routes"].items():
        assert g["files"]["out.csv"]["lines"] > 1, name                       # no route is pinned to an empty output


@pytest.mark.parametrize("name", ROUTE_NAMES)
def test_route_writes_and_logs_what_the_parent_did(runs, name):
    got, want = runs[name], GOLDEN["routes"][name]
    assert got["info"] == want["info"]
    assert got["stages"] == want["stages"]
    assert got["files"] == want["files"]


# ---- the API half ---------------------------------------------------------------------------------------------------------------------
def _cut(inp, how):
    """the alignment a call compares -> (seqs, names, kept columns, min_sites)"""
    seqs, isn = inp["seqs"], inp["isn"]
    if how == "nothing":
        return seqs, inp["names"], np.ones(T.L, bool), 0
    if how == "sites":
        cols = inp["keep"] & (isn[seqs].sum(axis=0) <= inp["max_n"])
        return seqs[:, cols], inp["names"], cols, 0
    samples, cols, _, _ = T.ruled_alignment(inp, isn)
    return seqs[samples][:, cols], [nm for nm, k in zip(inp["names"], samples) if k], cols, inp["min_sites"]


def _call(inp, fn, how):
    from tracs_amd import api
    f, head, kw = T.api_calls(inp, inp["min_sites"], inp["max_n"])["%s:%s" % (fn, how)]
    info = {}
    got = getattr(api, f)([inp["fa"]], *head, info=info, **kw)
    assert sorted(info) == GOLDEN["api_info_keys"]["%s:%s" % (fn, how)]
    return got, info


def _check_info(inp, info, how, cut):
    assert info["seqlen"] == cut.shape[1]
    if how == "rules":
        samples, _, counts, lp = T.ruled_alignment(inp, inp["isn"])
        assert info["source_names"] == inp["names"] and info["rule_sites"] == lp
        assert np.array_equal(info["n_counts"], counts) and np.array_equal(info["kept"], samples)


def _eligible(oracle, cut, dist, m):
    r, c, d, nn = oracle.pairsnp_arrays(cut, dist=dist)
    ok = nn >= m
    return r[ok], c[ok], d[ok], nn[ok]


@pytest.mark.parametrize("how", ["nothing", "sites", "rules"])
def test_api_pairsnp_arrays(inputs, oracle, how):
    cut, names, _, m = _cut(inputs, how)
    (r, c, d, got_names, f, nn), info = _call(inputs, "pairsnp_arrays", how)
    er, ec, ed, enn = _eligible(oracle, cut, inputs["dist"], m)
    assert got_names == names and len(er) > 0
    for g, e in zip((r, c, d, nn, f), (er, ec, ed, enn, oracle.filter_recomb_pairs(cut, er, ec))):
        assert np.array_equal(g, e)
    _check_info(inputs, info, how, cut)


@pytest.mark.parametrize("how", ["nothing", "sites", "rules"])
def test_api_nearest_arrays(inputs, oracle, how):
    cut, names, _, m = _cut(inputs, how)
    (r, c, d, got_names, _, nn), info = _call(inputs, "nearest_arrays", how)
    er, ec, ed, enn = _eligible(oracle, cut, inputs["dist"], m)
    er, ec, ed, enn = np.concatenate([er, ec]), np.concatenate([ec, er]), np.concatenate([ed, ed]), np.concatenate([enn, enn])
    o = np.lexsort((ec, ed, er))                        # each sample's partners by (distance, index), the first K
    er, ec, ed, enn = er[o], ec[o], ed[o], enn[o]
    top = np.arange(len(er)) - np.searchsorted(er, er) < T.K
    assert got_names == names and top.sum() > 0
    for g, e in zip((r, c, d, nn), (er[top], ec[top], ed[top], enn[top])):
        assert np.array_equal(g, e)
    _check_info(inputs, info, how, cut)


@pytest.mark.parametrize("how", ["nothing", "sites", "rules"])
def test_api_distance_histogram(inputs, oracle, how):
    from test_gpu_histogram import bincount_hist, check, classes_of
    cut, names, _, m = _cut(inputs, how)
    (got_names, hist), info = _call(inputs, "distance_histogram", how)
    er, ec, ed, _ = _eligible(oracle, cut, inputs["dist"], m)
    number = {None: -1, "g0": 0, "g1": 1, "g2": 2}
    labels = np.array([number[inputs["labels"][nm]] for nm in names], np.int64)
    assert got_names == names and set(hist) == {"snp"}
    check(hist["snp"], bincount_hist(ed, classes_of(labels, er, ec)), how)
    _check_info(inputs, info, how, cut)


@pytest.mark.parametrize("how", ["nothing", "sites", "rules"])
def test_api_pair_sites(inputs, oracle, hiplib, how):
    cut, names, cols, _ = _cut(inputs, how)
    (off, site, bits, got_names), info = _call(inputs, "pair_sites", how)
    masks = np.array([hiplib.tracs_debug_iupac_mask(ch) for ch in range(256)], np.uint32)[cut]
    pairs = T.api_calls(inputs, inputs["min_sites"], inputs["max_n"])["pair_sites:" + how][1][0]
    idx = [tuple(names.index(x) if isinstance(x, str) else x for x in p) for p in pairs]
    want_site = [np.flatnonzero((masks[a] & masks[b]) == 0) for a, b in idx]
    assert got_names == names and np.array_equal(off, np.concatenate([[0], np.cumsum([len(s) for s in want_site])]))
    assert np.array_equal(site, np.concatenate(want_site)) and len(site) > 0
    assert np.array_equal(bits & 0xFF, np.concatenate([masks[a, s] | (masks[b, s] << 4) for (a, b), s in zip(idx, want_site)]))
    lo, hi = [min(p) for p in idx], [max(p) for p in idx]
    kept = [int(((bits[off[t]:off[t + 1]] >> 8) == 0).sum()) for t in range(len(idx))]
    assert kept == oracle.filter_recomb_pairs(cut, lo, hi).astype(np.int64).tolist()
    assert np.array_equal(info["positions"], np.flatnonzero(cols))
    _check_info(inputs, info, how, cut)
