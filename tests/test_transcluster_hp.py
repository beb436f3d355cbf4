"""tests/golden/transcluster_hp_golden.json -- transcluster's p0 and E(K) from the series' definition at 40 digits -- against a
fresh high-precision evaluation (a seeded sample), and the oracle (oracle/tracs_oracle.c, the reference's loop in double) against
the fixture where the reference's lgamma table still holds the key (N <= 3 000)."""
import json
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "golden", "transcluster_hp_golden.json")


def _keys():
    with open(FIXTURE) as fh:
        f = json.load(fh)
    return [dict(zip(f["fields"], r)) for r in f["keys"]], f["sets"]


def _close_log(a, b, tol):
    if a == b:
        return True
    return abs(a - b) <= tol * max(1.0, abs(b))


def test_fixture_covers_the_domain():
    keys, sets = _keys()
    Ns = {k["N"] for k in keys}
    for n in (0, 127, 128, 191, 192, 9998, 10001, 22766, 22767, 32767, 32768, 100000):
        assert n in Ns
    for s in range(len(sets)):                    # every N boundary in every (lamb, beta, thr) set
        assert {k["N"] for k in keys if k["set"] == s} == Ns
    gaps = {k["gap"] for k in keys if k["set"] == 0}
    assert {0, 1, 2, 30, 365, 730, 1000, 2400, 9000, None} <= gaps
    assert {k["cls"] for k in keys} == {"determined", "saturated", "ill"}
    for k in keys:
        if k["gap"] is not None:
            assert k["delta"] == k["gap"] * 86400.0 / 31556952.0
        assert k["k_lo"] <= k["k_stop"] <= k["k_hi"] <= 9999
        assert (k["cls"] == "ill") == (k["k_lo"] != k["k_hi"])


def test_recomputed_keys_equal_the_fixture():
    pytest.importorskip("mpmath")
    import hp_transcluster as H
    keys, sets = _keys()
    small = [k for k in keys if k["N"] <= 2000]
    rng = np.random.default_rng(7)
    for i in rng.choice(len(small), 24, replace=False):
        k = small[int(i)]
        lamb, beta, thr = sets[k["set"]]
        r = H.evaluate(k["N"], k["delta"], lamb, beta, thr)
        for f in ("k_stop", "cls", "k_lo", "k_hi"):
            assert r[f] == k[f], (k, f, r[f])
        for f in ("p0", "ln_eK", "ln_e_lo", "ln_e_hi", "ln_upper"):
            assert _close_log(r[f], k[f], 1e-15), (k, f, r[f])


def test_oracle_matches_the_fixture():
    from oracle import oracle as O
    keys, sets = _keys()
    # (the oracle's loop costs k_stop (N + k_stop) lgamma terms: every key of short loops, and a seeded sample of the long ones)
    mine = [k for k in keys if k["N"] <= 3000]
    cheap = [k for k in mine if k["k_hi"] * (k["N"] + k["k_hi"]) <= 4e6]
    dear = [k for k in mine if k["k_hi"] * (k["N"] + k["k_hi"]) > 4e6]
    rng = np.random.default_rng(11)
    todo = cheap + [dear[int(i)] for i in rng.choice(len(dear), 8, replace=False)]
    worst_p0 = worst_ek = 0.0
    checked = 0
    for k in todo:
        lamb, beta, thr = sets[k["set"]]
        p0, ek = O.trans_dist([k["N"]], [k["delta"]], lamb, beta, thr)
        assert _close_log(float(p0[0]), k["p0"], 1e-12), k
        worst_p0 = max(worst_p0, abs(float(p0[0]) - k["p0"]) / max(1.0, abs(k["p0"])))
        cond = O.ek_conditioning(k["N"], k["delta"], lamb, beta, thr)[0]
        if cond == "well":
            assert k["cls"] == "determined", (k, cond)
        elif cond == "saturated":
            assert k["cls"] == "saturated", (k, cond)
        if k["cls"] == "ill":
            continue
        want = k["ln_eK"]
        if want < math.log(1e-290):
            assert float(ek[0]) <= 1e-290, k
            continue
        rel = abs(float(ek[0]) / math.exp(want) - 1.0)
        assert rel <= 1e-10, (k, float(ek[0]), math.exp(want))
        worst_ek = max(worst_ek, rel)
        checked += 1
    assert checked > 60
    print("oracle vs high precision: p0 %.3g, E(K) %.3g (relative)" % (worst_p0, worst_ek))
