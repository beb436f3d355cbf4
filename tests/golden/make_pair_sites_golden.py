"""Writes tests/golden/pair_sites_hp_golden.json: for the crafted pairs of tests/golden/filter_hp_golden.json with L in {9000, 120000}
-- the boundary positions and both probes of each case, 45 pairs -- the recombination filter's decision for EVERY SNP, from the
definition at 50 digits (tests/hp_filter.py): a SNP is kept when its window holds at most one SNP, otherwise by the cell
(count, length) of hp_filter.filter_positions.  The fixture's `row` alone cannot give these flags: some windows hold 64 SNPs or more,
and the rows end at 63.

One hex string per pair: bit u & 7 of byte u >> 3 is 1 when the pair's u-th SNP (in site order) is kept.  Pairs are in the order of
the samples 1, 2, .. of tests/test_gpu_filter_hp.py's alignments: per case the boundary sites, the probe at wh, the probe at wh + 1.

    python tests/golden/make_pair_sites_golden.py          (needs mpmath and scipy, as hp_filter does)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
LENGTHS = (9000, 120000)


def kept_flags(H, pos, L):
    """-> (bool[d] kept per SNP, ill cells) from the definition: filter_positions' windows, decided per SNP"""
    pos = np.asarray(pos, np.int64)
    d = len(pos)
    if d <= 1:
        return np.ones(d, bool), 0
    total, cells, ill, _ = H.filter_positions(pos, L)
    _, _, wh = H.window(L, d)
    lo = np.searchsorted(pos, np.maximum(0, pos - wh), "left")
    hi = np.searchsorted(pos, np.minimum(L, pos + wh + 1), "left")
    count = hi - lo
    length = pos[hi - 1] - pos[lo] + 1
    flags = np.array([c <= 1 or cells[(int(c), int(n))] for c, n in zip(count, length)], bool)
    assert int(flags.sum()) == total
    return flags, ill


def pairs_of(H, case):
    """[(kind, sites, expected kept)] of one fixture case, in sample order"""
    L, d = case["L"], case["d"]
    shape, at_wh, beyond = case["probe"]
    return [("boundary", H.boundary_positions(L, d, case["row"]), case["expected"]),
            ("probe_wh", H.probe_positions(L, d, shape, case["wh"]), at_wh),
            ("probe_wh1", H.probe_positions(L, d, shape, case["wh"] + 1), beyond)]


def to_hex(flags):
    return np.packbits(np.asarray(flags, bool), bitorder="little").tobytes().hex()


def from_hex(text, d):
    return np.unpackbits(np.frombuffer(bytes.fromhex(text), np.uint8), bitorder="little")[:d].astype(bool)


def make():
    import hp_filter as H
    with open(os.path.join(HERE, "filter_hp_golden.json")) as fh:
        cases = [c for c in json.load(fh)["cases"] if c["L"] in LENGTHS]
    pairs, snps = [], 0
    for c in cases:
        for kind, pos, expected in pairs_of(H, c):
            flags, ill = kept_flags(H, pos, c["L"])
            assert ill == 0, (c["L"], c["d"], kind)
            assert int(flags.sum()) == expected, (c["L"], c["d"], kind, int(flags.sum()), expected)
            pairs.append({"L": c["L"], "d": c["d"], "kind": kind, "kept": int(flags.sum()), "flags": to_hex(flags)})
            snps += len(pos)
    return {"about": "per-SNP kept flags of the recombination filter for the crafted pairs of filter_hp_golden.json (L = 9000, 120000), "
                     "from the definition at 50 digits (tests/hp_filter.py); bit u & 7 of byte u >> 3 of `flags`: SNP u is kept",
            "digits": H.DPS, "pairs_total": len(pairs), "snps_total": snps, "pairs": pairs}


if __name__ == "__main__":
    import time
    t0 = time.time()
    out = make()
    path = os.path.join(HERE, "pair_sites_hp_golden.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")
    print("%s: %d pairs, %d SNPs, %.2f s" % (path, out["pairs_total"], out["snps_total"], time.time() - t0))
