"""tests/golden/pair_sites_hp_golden.json -- the recombination filter's decision for every SNP of the crafted pairs of
filter_hp_golden.json with L in {9000, 120000}, from the definition at 50 digits (tests/golden/make_pair_sites_golden.py) -- against
that fixture's filtered distances on every pair, and against a fresh evaluation of a sample of it, as tests/test_filter_hp.py does
for its own fixture.  The GPU tests (tests/test_gpu_pair_sites.py) read the flags; they evaluate nothing in high precision."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
FIXTURE = os.path.join(HERE, "golden", "pair_sites_hp_golden.json")
SOURCE = os.path.join(HERE, "golden", "filter_hp_golden.json")


@pytest.fixture(scope="module")
def fx():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def cases():
    with open(SOURCE) as fh:
        return [c for c in json.load(fh)["cases"] if c["L"] in (9000, 120000)]


@pytest.fixture(scope="module")
def M():
    pytest.importorskip("mpmath")
    import hp_filter
    import make_pair_sites_golden
    return make_pair_sites_golden, hp_filter


def test_fixture_shape_and_sums(fx, cases):
    """45 pairs and 42 255 SNPs in the order of the alignments' samples; the flags of every pair sum to the source fixture's filtered
    distance (the boundary sites) or probe value"""
    import make_pair_sites_golden as G
    assert fx["digits"] >= 40 and fx["pairs_total"] == len(fx["pairs"]) == 3 * len(cases) == 45
    assert fx["snps_total"] == sum(p["d"] for p in fx["pairs"]) == 42255
    want = []
    for c in cases:
        want += [(c["L"], c["d"], "boundary", c["expected"]), (c["L"], c["d"], "probe_wh", c["probe"][1]),
                 (c["L"], c["d"], "probe_wh1", c["probe"][2])]
    assert [(p["L"], p["d"], p["kind"], p["kept"]) for p in fx["pairs"]] == want
    for p in fx["pairs"]:
        flags = G.from_hex(p["flags"], p["d"])
        assert len(flags) == p["d"] and int(flags.sum()) == p["kept"], (p["L"], p["d"], p["kind"])
        assert len(p["flags"]) == 2 * ((p["d"] + 7) // 8) and G.to_hex(flags) == p["flags"]      # (no stray bits behind the last SNP)
    assert any(0 < p["kept"] < p["d"] for p in fx["pairs"])


def test_the_rows_alone_cannot_give_the_flags(fx, cases, M):
    """some windows of the crafted pairs hold 64 SNPs or more, beyond the counts filter_hp_golden.json's rows cover"""
    G, H = M
    big = 0
    for c in cases:
        pos = np.asarray(H.boundary_positions(c["L"], c["d"], c["row"]), np.int64)
        if len(pos) < 2:
            continue
        _, _, wh = H.window(c["L"], c["d"])
        count = np.searchsorted(pos, np.minimum(c["L"], pos + wh + 1), "left") - np.searchsorted(pos, np.maximum(0, pos - wh), "left")
        big += int((count > H.K_HI).sum())
    assert big > 0


def test_generator_reproduces_a_sample(fx, cases, M):
    """the flags of a sample of the pairs, evaluated afresh at 50 digits: no ill cell, the same bits"""
    G, H = M
    by_case = {(c["L"], c["d"]): c for c in cases}
    rng = np.random.default_rng(11)
    edges = [(9000, 90), (9000, 91), (120000, 1200), (120000, 1201)]
    rest = sorted(set(by_case) - set(edges))
    todo = edges + [rest[int(i)] for i in rng.choice(len(rest), 4, replace=False)]
    stored = {(p["L"], p["d"], p["kind"]): p for p in fx["pairs"]}
    for key in todo:
        c = by_case[key]
        for kind, pos, expected in G.pairs_of(H, c):
            flags, ill = G.kept_flags(H, pos, c["L"])
            p = stored[c["L"], c["d"], kind]
            assert ill == 0 and int(flags.sum()) == expected == p["kept"], (key, kind)
            assert G.to_hex(flags) == p["flags"], (key, kind)
