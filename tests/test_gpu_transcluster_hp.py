"""Every transcluster route against tests/golden/transcluster_hp_golden.json (p0 and E(K) from the series' definition at 40
digits, tests/hp_transcluster.py), at N up to 100 000, day gaps up to 9 000 and seven (lamb, beta, thr) sets.  Each call asserts the
route it was meant to take (device.trans_routes): the array entry points, the dense block with linear (gap, M) tables, with tables
in log space, without tables, the hash route (TRACS_TC_GRID=0, a child process), the key split over three ranks on one GPU and the
key-table route (device.trans_dist_dense_partitioned) with three parts played in turn.

Tolerances: p0 |d ln P| <= 1e-12 max(1, |ln P|).  E(K) of determined and saturated keys: relative <= max(1e-10, 4e-16 lgG(N +
k_stop + 1)) -- the rounding of the reference formula's largest log term -- where the exact value is >= 1e-290, else <= 1e-290.
'ill' keys (the stop decided by rounding): between the exact partial sums at k_lo and k_hi, with the same tolerance."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(HERE, "golden", "transcluster_hp_golden.json")
LN_TINY = math.log(1e-290)
WORST = {}                      # route -> class -> worst deviation (relative; p0 under "p0")


def _fixture():
    with open(FIXTURE) as fh:
        f = json.load(fh)
    return [dict(zip(f["fields"], r)) for r in f["keys"]], [tuple(s) for s in f["sets"]]


def _ek_tol(k):
    return max(1e-10, 4e-16 * math.lgamma(k["N"] + k["k_stop"] + 1))


def _note(route, cls, v):
    w = WORST.setdefault(route, {})
    w[cls] = max(w.get(cls, 0.0), float(v))


def _check(route, keys, p0, ek):
    """p0 (log) and E(K) of `keys`, one value each, against the fixture"""
    bad = []
    for k, a, e in zip(keys, np.asarray(p0, np.float64), np.asarray(ek, np.float64)):
        a, e = float(a), float(e)
        dp = abs(a - k["p0"]) / max(1.0, abs(k["p0"]))
        _note(route, "p0", dp)
        if not dp <= 1e-12:
            bad.append(("p0", k, a))
        tol = _ek_tol(k)
        if k["cls"] in ("determined", "saturated"):
            if k["ln_eK"] < LN_TINY:
                ok = e <= 1e-290
            else:
                rel = abs(e / math.exp(k["ln_eK"]) - 1.0)
                _note(route, k["cls"], rel)
                ok = rel <= tol
        else:
            lo = math.exp(k["ln_e_lo"]) if k["ln_e_lo"] >= LN_TINY else 0.0
            hi = math.exp(k["ln_e_hi"]) if k["ln_e_hi"] >= LN_TINY else 1e-290
            ok = lo * (1 - tol) <= e <= hi * (1 + tol)
        if not ok:
            bad.append(("eK", k, e))
    assert not bad, "%s: %d of %d keys off, first: %r" % (route, len(bad), len(keys), bad[:3])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\ntranscluster vs high precision, worst deviation per route and class:")
        for r, w in sorted(WORST.items()):
            print("  %-14s %s" % (r, "  ".join("%s %.3g" % kv for kv in sorted(w.items()))))
        out = os.environ.get("TRACS_REPORT_DIR")          # (also as JSON, when a report directory is named)
        if out:
            os.makedirs(out, exist_ok=True)
            with open(os.path.join(out, "transcluster_hp.json"), "w") as fh:
                json.dump(WORST, fh, indent=1, sort_keys=True)


# ---- the array entry points: every key of every set, deltas of whole days and others ------------------------------------------
def test_array_routes_match_high_precision():
    import torch
    from tracs_amd import api
    from tracs_amd import device as dev
    keys, sets = _fixture()
    seen = {"serial": 0, "ratio_zero": 0, "wave": 0}
    for s, (lamb, beta, thr) in enumerate(sets):
        ks = [k for k in keys if k["set"] == s]
        N = np.array([k["N"] for k in ks], np.int32)
        d = np.array([k["delta"] for k in ks], np.float64)
        p0, ek = api.trans_dist_arrays(N, d, lamb, beta, thr)
        r = dev.trans_routes()
        assert r["keys"] == len(set(zip(N.tolist(), d.tolist()))) and r["route"] == "hash" and not r["tables"]
        # (no tables without day gaps: no term-ratio loop; the same-day one needs none)
        assert r["ratio"] == 0 and r["serial"] + r["ratio_zero"] + r["wave"] == r["keys"], r
        for f in seen:
            seen[f] += r[f]
        _check("array", ks, p0, ek)
        p0d, ekd = dev.trans_dist_device(torch.from_numpy(N).cuda(), torch.from_numpy(d).cuda(), lamb, beta, thr)
        assert dev.trans_routes() == r
        _check("device", ks, p0d.cpu().numpy(), ekd.cpu().numpy())
    assert min(seen.values()) > 0, seen


# ---- dense blocks: sample 0 on day 0, a sample per fixture key on day `gap` with d[0, i] = N, filler cells beside them ---------
DENSE = {
    # name: (largest gap, largest N, filler: None = one constant (few keys), else the largest filler N)
    "linear": (730, 22769, 2000),           # term-ratio loop up to N = 22 766, the log-space wave beyond; same-day ratio loop
    "linear_wide": (1000, 15000, 2000),
    "log": (2400, 6000, 2000),              # x = delta (lamb + beta) = 676 > 600: tables in log space
    "untabled": (9000, 100000, None),       # tables too large: nothing tabled; keys beyond the grid: hash route
    "few_keys": (9000, 1600, None),         # fewer than 2 048 keys: no tables, grid route
}


def _dense_case(name):
    gap_max, n_max, fill = DENSE[name]
    keys, sets = _fixture()
    ks = [k for k in keys if k["set"] == 0 and k["gap"] is not None and k["gap"] <= gap_max and k["N"] <= n_max]
    days = [0] + [k["gap"] for k in ks]
    rng = np.random.default_rng(gap_max + n_max)
    if fill is not None:
        # enough distinct keys that the tables pay, (gap_max + 1) (n_max + 10 001) <= 4 096 keys, also for a third of them (key split)
        need = (gap_max + 1) * (n_max + 10001) / 4096.0
        while len(days) * (len(days) - 1) / 2 < 3.6 * need + 2048:
            days.append(int(rng.integers(0, gap_max + 1)))
    n = len(days)
    if fill is None:
        d = np.zeros((n, n), np.int64)
    else:
        d = rng.integers(0, fill + 1, size=(n, n))
    d[0, 1:1 + len(ks)] = [k["N"] for k in ks]
    d = np.triu(d, 1)
    d = (d + d.T).astype(np.int32)
    return ks, sets[0], d, np.array(days, np.int32)


def _dense_run(name):
    """-> (p0 row 0 (log), E(K) row 0, routes) of one trans_dist_dense_ranges call over the whole block"""
    import torch
    from tracs_amd import device as dev
    ks, (lamb, beta, thr), d, days = _dense_case(name)
    n = d.shape[0]
    dm, dy = torch.from_numpy(d).cuda(), torch.from_numpy(days).cuda()
    p = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
    e = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
    dev.trans_dist_dense_ranges(dm, n, dy, lamb, beta, thr, p, e, [(0, n)], exp_p0=False)
    r = dev.trans_routes()
    m = len(ks)
    return p[0, 1:1 + m].cpu().numpy(), e[0, 1:1 + m].cpu().numpy(), r


def _distinct(name):
    _, _, d, days = _dense_case(name)
    iu = np.triu_indices(d.shape[0], 1)
    return len(set(zip(d[iu].tolist(), np.abs(days[iu[0]] - days[iu[1]]).tolist())))


@pytest.mark.parametrize("name", sorted(DENSE))
def test_dense_routes_match_high_precision(name):
    ks = _dense_case(name)[0]
    p0, ek, r = _dense_run(name)
    assert r["keys"] == _distinct(name)
    assert r["serial"] + r["ratio"] + r["ratio_zero"] + r["wave"] == r["keys"]
    assert r["serial"] > 0 and r["wave"] > 0, r
    if name.startswith("linear"):
        assert r["tables"] and r["linear"] and r["route"] == "grid" and r["ratio"] > 0 and r["ratio_zero"] > 0, r
    elif name == "log":
        assert r["tables"] and not r["linear"] and r["route"] == "grid" and r["ratio"] == 0 and r["ratio_zero"] > 0, r
    elif name == "untabled":
        assert not r["tables"] and r["route"] == "hash" and r["ratio"] == 0, r
        assert max(k["N"] for k in ks) == 100000 and max(k["gap"] for k in ks) == 9000
    else:
        assert r["keys"] < 2048 and not r["tables"] and r["route"] == "grid", r
    _check("dense_" + name, ks, p0, ek)


HASH_CHILD = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import json
import numpy as np
import test_gpu_transcluster_hp as T
p0, ek, r = T._dense_run("linear")
np.savez(sys.argv[1], p0=p0, ek=ek)
json.dump(r, open(sys.argv[1] + ".json", "w"))
'''


def test_hash_route_matches_high_precision(tmp_path):
    """The block of the 'linear' case with the grid route off (TRACS_TC_GRID=0 is read once per process: a child)."""
    f = os.path.join(str(tmp_path), "hash.npz")
    out = subprocess.run([sys.executable, "-c", HASH_CHILD % {"root": ROOT, "tests": HERE}, f], capture_output=True, text=True,
                         env=dict(os.environ, TRACS_TC_GRID="0"), timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    z = np.load(f)
    with open(f + ".json") as fh:
        r = json.load(fh)
    assert r["route"] == "hash" and r["tables"] and r["linear"] and r["ratio"] > 0 and r["ratio_zero"] > 0 and r["wave"] > 0, r
    _check("dense_hash", _dense_case("linear")[0], z["p0"], z["ek"])


def test_key_split_matches_high_precision():
    """partition.KeySplit's kernels, three ranks played one after the other (tests/test_gpu_keysplit.py): each rank evaluates its
    share of the distinct keys of the 'linear_wide' block, and gathers its own rows; row 0's cells against the fixture."""
    import torch
    from tracs_amd import device as dev
    from tracs_amd import partition
    ks, (lamb, beta, thr), d, days = _dense_case("linear_wide")
    n, world = d.shape[0], 3
    dm, dy = torch.from_numpy(d).cuda(), torch.from_numpy(days).cuda()
    own = [partition.own_row_ranges(0, n, q, world) for q in range(world)]
    words = dev.trans_keys_words()
    gathered = torch.empty(world * words, dtype=torch.int32, device="cuda")
    masks = []
    for q in range(world):
        mine = torch.zeros(n, dtype=torch.bool, device="cuda")
        for r0, r1 in own[q]:
            mine[r0:r1] = True
        masks.append(mine)
        dq = torch.where(mine[:, None], dm, torch.full_like(dm, 77777))
        dev.trans_keys_mark(dq, n, dy, own[q], gathered[q * words:(q + 1) * words])
    union = torch.empty(words, dtype=torch.int32, device="cuda")
    dev.trans_keys_merge(union, gathered, world)
    info = dev.trans_keys_info(union)
    assert info[3] == 1 and info[0] == _distinct("linear_wide")
    per = max(1, -(-info[0] // world))
    vals_all = torch.full((world * per * 2,), float("nan"), dtype=torch.float64, device="cuda")
    evaluated = 0
    for q in range(world):
        dev.trans_keys_evaluate(union, info, q, world, lamb, beta, thr, vals_all[q * per * 2:(q + 1) * per * 2])
        r = dev.trans_routes()
        assert r["route"] == "grid" and r["tables"] and r["linear"], r
        evaluated += r["keys"]
    assert evaluated == info[0]
    p0 = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
    ek = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
    for q in range(world):
        pq = torch.full_like(p0, float("nan"))
        eq = torch.full_like(ek, float("nan"))
        dq = torch.where(masks[q][:, None], dm, torch.full_like(dm, 77777))
        dev.trans_keys_gather(dq, n, dy, own[q], union, info, vals_all, world, pq, eq, exp_p0=False)
        p0[masks[q]] = pq[masks[q]]
        ek[masks[q]] = eq[masks[q]]
    m = len(ks)
    _check("keysplit", ks, p0[0, 1:1 + m].cpu().numpy(), ek[0, 1:1 + m].cpu().numpy())


def test_key_table_matches_high_precision():
    """device.trans_dist_dense_partitioned (the key-table route of several ranks), three parts played one after the other
    (tests/test_gpu_key_table.py: the all-reduce is the sum of the parts' tables) on the 'linear' block: every part's row 0 against
    the fixture."""
    import torch
    from test_gpu_key_table import play_parts
    from tracs_amd import device as dev
    ks, (lamb, beta, thr), d, days = _dense_case("linear")
    n, parts = d.shape[0], 3
    dm, dy = torch.from_numpy(d).cuda(), torch.from_numpy(days).cuda()
    got = play_parts(dev, dm, n, dy, lamb, beta, thr, parts, False, 2147483647, n)
    # (keys / tables / linear describe all the parts' keys together: tests/test_gpu_key_table.py)
    r = dev.trans_routes()
    assert r["keys"] == _distinct("linear") and r["route"] == "hash" and r["tables"] and r["linear"], r
    m = len(ks)
    for p0, ek in got:
        _check("keytable", ks, p0[0, 1:1 + m].cpu().numpy(), ek[0, 1:1 + m].cpu().numpy())
