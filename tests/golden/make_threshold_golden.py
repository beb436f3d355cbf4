#!/usr/bin/env python3
"""Generate tests/golden/threshold_golden.json (run in the build container only).

Source of truth: the reference's own tracs/threshold.py, loaded from the reference tree when this script runs -- its negbinom_ll,
its mixture and its optimizer_NM, on the RAW list of distances.  The reference hands +sum(log-likelihood) of the mixture to its
minimiser (tracs/threshold.py:63-67, 98); the fit it intends, and the one recorded here, minimises `mixture` NEGATED.
Only DATA is written: per case the two samples as (value, count) lists, the reference's r, p, q, lambda and threshold, and `spread`,
the largest absolute change of each parameter when the same raw list is given in three orders (as generated, ascending, descending)
-- how far the reference's own answer moves with the order of summation.

A case must keep the comparison meaningful, or it is replaced (never loosened): both reference fits report success; r < 1e4 (towards
the Poisson limit r and p are not separately determined); poisson.ppf(0.95, lambda') is the same for every lambda' within 1e-3 of
lambda (the threshold does not sit on a step of the quantile).
"""
import importlib.util
import json
import os
import sys

import numpy as np
import scipy.optimize as optimize
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("TRACS_REFERENCE", "/root/reference")


def reference_threshold():
    spec = importlib.util.spec_from_file_location("tracs_reference_threshold", os.path.join(REF, "tracs", "threshold.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = reference_threshold()


def reference_fit(close, distant):
    """r, p, q, lambda, threshold by the reference's functions on raw lists, and whether both minimisations report success."""
    close, distant = np.asarray(close, dtype=float), np.asarray(distant, dtype=float)
    f_far = lambda params: T.negbinom_ll(params, distant)                      # noqa: E731
    r, p = T.optimizer_NM(f_far, np.array([100, 0.5]))
    f_mix = lambda params: -T.mixture(params, close, r, p)                     # noqa: E731
    with np.errstate(all="ignore"):
        q, lambd = T.optimizer_NM(f_mix, np.array([0.5, 1]))
        ok = bool(optimize.minimize(f_far, np.array([100, 0.5]), method="nelder-mead").success and
                  optimize.minimize(f_mix, np.array([0.5, 1]), method="nelder-mead").success)
    return np.array([r, p, q, lambd]), float(stats.poisson.ppf(0.95, mu=lambd) * 3), ok


def histogram(values):
    v, c = np.unique(np.asarray(values, dtype=np.int64), return_counts=True)
    return [[int(a), int(b)] for a, b in zip(v, c)]


def case(name, close, distant, note):
    close, distant = np.asarray(close, dtype=np.int64), np.asarray(distant, dtype=np.int64)
    fits = []
    for order in (lambda x: x, np.sort, lambda x: np.sort(x)[::-1]):
        fits.append(reference_fit(order(close), order(distant)))
    par, thr, ok = fits[0]
    assert all(f[2] for f in fits), (name, "a reference fit did not report success")
    assert all(f[1] == thr for f in fits), (name, "the threshold depends on the order of the raw list")
    assert par[0] < 1e4, (name, "r is in the Poisson limit", par)
    assert 0 < par[2] < 1 and par[3] > 0, (name, par)
    lam = par[3]
    assert len({float(stats.poisson.ppf(0.95, mu=x)) for x in np.linspace(lam - 1e-3, lam + 1e-3, 41)}) == 1, (name, "threshold on a step", lam)
    spread = np.max(np.abs(np.array([f[0] for f in fits]) - par), axis=0)
    print("%-12s r=%.6g p=%.6g q=%.6g lambda=%.6g threshold=%g spread=%s n_close=%d n_distant=%d"
          % (name, par[0], par[1], par[2], par[3], thr, spread.tolist(), len(close), len(distant)))
    return {"name": name, "note": note, "close": histogram(close), "distant": histogram(distant),
            "r": float(par[0]), "p": float(par[1]), "q": float(par[2]), "lambda": float(par[3]), "snp_threshold": thr,
            "spread": {k: float(s) for k, s in zip(("r", "p", "q", "lambda"), spread)}}


def simulated(rng, r, p, n_distant, n_close, frac, lam):
    distant = rng.negative_binomial(r, p, n_distant)
    k = int(round(n_close * frac))
    close = np.concatenate([rng.poisson(lam, k), rng.negative_binomial(r, p, n_close - k)])
    return rng.permutation(close), distant


def grouped_alignment(rng, n_lineages=12, per_lineage=20, L=20000):
    """An alignment whose between-lineage distances are over-dispersed (every lineage has a mutation rate of its own, drawn from a
    range) and whose groups are mostly one lineage plus a few strangers.  -> seqs uint8[n, L], group label per sample."""
    bases = np.frombuffer(b"ACGT", np.uint8)
    anc = rng.integers(0, 4, L)

    def mutate(code, rate):
        out = code.copy()
        hit = rng.random(L) < rate
        out[hit] = (out[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        return out
    seqs, label = [], []
    for g in range(n_lineages):
        founder = mutate(anc, rng.uniform(2e-3, 1.5e-2))
        for _ in range(per_lineage):
            seqs.append(mutate(founder, 2e-4))
            label.append(g)
    label = np.array(label)
    strangers = rng.choice(len(label), 3 * n_lineages, replace=False)          # a few samples filed under another lineage's group
    label[strangers] = (label[strangers] + rng.integers(1, n_lineages, len(strangers))) % n_lineages
    return bases[np.array(seqs)], label


def main():
    from oracle import oracle as O
    rng = np.random.default_rng(20250611)
    cases = []
    close, distant = simulated(rng, 20, 0.02, 20000, 3000, 0.3, 3.0)
    cases.append(case("simulated", close, distant, "distant NB(20, 0.02) x 20000; close 3000, 30 % Poisson(3), the rest NB(20, 0.02)"))
    seqs, label = grouped_alignment(rng)
    rows, cols, d, _ = O.pairsnp_arrays(seqs, n_threads=8)
    same = label[rows.astype(np.int64)] == label[cols.astype(np.int64)]
    cases.append(case("alignment", d[same], d[~same], "240 x 20000 alignment, 12 lineages with rates in [2e-3, 1.5e-2], groups with strangers; "
                                                      "all pairs by the CPU oracle"))
    close, distant = simulated(rng, 5, 0.01, 5000, 100, 0.5, 4.0)
    cases.append(case("few_close", close, distant, "distant NB(5, 0.01) x 5000; close 100, half Poisson(4)"))
    with open(os.path.join(HERE, "threshold_golden.json"), "w") as fh:
        # one case per line block, the (value, count) lists on one line each: data a reader can scan
        fh.write('{"cases": [\n')
        for k, c in enumerate(cases):
            fh.write(" {\n" + ",\n".join("  %s: %s" % (json.dumps(key), json.dumps(val)) for key, val in c.items()) + "\n }"
                     + (",\n" if k + 1 < len(cases) else "\n"))
        fh.write("]}\n")
    print("wrote threshold_golden.json")


if __name__ == "__main__":
    main()
