"""Shared by the sample-rule tests: the standard input of the site-rule tests with the rule's edge cases planted,
and the expected result of the three rules in numpy.  "Is N" is the library's own letter table (site_rules_common.is_n_table)."""
import math

import numpy as np

from site_rules_common import standard_files_keep, standard_input

G, F = 0.1, 0.05                      # --max-sample-n-share, --max-n-share of the standard case
SPECIAL = slice(400, 410)             # columns at which exactly the dropped samples are N (kept by the files, outside the N runs)


def files_keep(L):
    """the file rule of these tests: the standard mask plus one block of L / 5 columns -> bool[L], True = may stay.  The block makes
    the masked columns several times floor(G L'): a sample that is N there and nowhere else must stay"""
    keep = standard_files_keep(L)
    keep[L // 2:L // 2 + L // 5] = False
    return keep


def expected(seqs, isn, keep=None, g=None, f=None):
    """The three rules in their order -> dict: rule_sites L', threshold T, n_counts per record (over the file-kept columns),
    kept_samples bool[n], kept_sites bool[L] (file rules, then the N share over the SURVIVING samples)."""
    n, L = seqs.shape
    keep = np.ones(L, bool) if keep is None else np.asarray(keep, bool)
    lp = int(keep.sum())
    is_n = isn[seqs]
    counts = is_n[:, keep].sum(axis=1)
    t = math.floor(g * lp) if g is not None else lp
    kept_samples = counts <= t
    kept_sites = keep.copy()
    if f is not None:
        n_left = int(kept_samples.sum())
        kept_sites &= is_n[kept_samples].sum(axis=0) <= math.floor(f * n_left)
    return dict(rule_sites=lp, threshold=t, n_counts=counts, kept_samples=kept_samples, kept_sites=kept_sites)


def planted_input(n, L, isn, n_query=None, seed=11, with_files=True):
    """standard_input with the edge cases of the sample rule planted -> (seqs, keep or None, plan).  T = floor(G L'):
      stays_exact      a sample with exactly T N among the file-kept columns
      goes_exact       one with T + 1
      stays_masked     one that is N at EVERY masked column and stays (with_files only: a count that ignores the bitmap drops it)
      dropped          the first and last record of each file (n_query: the records [0, n_query) are the first file), goes_exact,
                       and seven more, all with more than T
      SPECIAL          columns at which exactly the dropped samples are N: over all samples more than floor(F n) -- the columns
                       go if the N share is counted before the sample rule --, over the survivors none"""
    seqs, _ = standard_input(n, L, seed)
    keep = files_keep(L) if with_files else None
    kcols = np.ones(L, bool) if keep is None else keep
    lp = int(kcols.sum())
    t = math.floor(G * lp)
    rng = np.random.default_rng(seed + 77)
    nq = n if n_query is None else n_query
    plan = dict(stays_exact=3, goes_exact=5, stays_masked=7 if with_files else None, T=t, rule_sites=lp)
    dropped = sorted({0, 5, 9, 11, 13, 15, 17, 19, nq - 1, nq % n, n - 1})
    plan["dropped"] = dropped
    special = np.zeros(L, bool)
    special[SPECIAL] = True
    assert kcols[special].all()
    free = np.flatnonzero(kcols & ~special)
    block = seqs[:, special]
    block[isn[block]] = ord("C")
    seqs[:, special] = block
    for s in dropped:
        seqs[s, special] = ord("N")

    def set_count(s, count):
        """sample s: exactly `count` N among the file-kept columns (its SPECIAL columns stay as they are)"""
        row = seqs[s]
        row[np.flatnonzero(isn[row] & kcols & ~special)] = ord("A")
        have = int((isn[row] & kcols).sum())
        assert have <= count
        row[rng.choice(free, count - have, replace=False)] = ord("N")
    for s in dropped:
        set_count(s, t + 1 if s == plan["goes_exact"] else t + 40 + 3 * s)
    set_count(plan["stays_exact"], t)
    if with_files:
        seqs[plan["stays_masked"], ~keep] = ord("-")
    return seqs, keep, plan


def check_plan(seqs, isn, keep, plan, n_query=None):
    """the planted cases are what they claim to be (every GPU test asserts its own non-vacuity through this)"""
    n, L = seqs.shape
    e = expected(seqs, isn, keep, G, F)
    t = plan["T"]
    assert e["threshold"] == t and e["rule_sites"] == plan["rule_sites"]
    assert e["n_counts"][plan["stays_exact"]] == t and e["kept_samples"][plan["stays_exact"]]
    assert e["n_counts"][plan["goes_exact"]] == t + 1 and not e["kept_samples"][plan["goes_exact"]]
    gone = np.flatnonzero(~e["kept_samples"]).tolist()
    assert gone == plan["dropped"] and 1 <= len(gone) <= n - 2
    assert 0 in gone and n - 1 in gone
    if n_query is not None:
        assert n_query - 1 in gone and n_query in gone
    if keep is not None:
        s = plan["stays_masked"]
        assert e["kept_samples"][s] and isn[seqs[s]][~keep].all() and (~keep).sum() > 2 * t      # dropped by a count over every column
    # the SPECIAL columns: kept only when the N share is counted over the survivors
    is_n = isn[seqs]
    assert (is_n[:, SPECIAL].sum(axis=0) > math.floor(F * n)).all() and e["kept_sites"][SPECIAL].all()
    kcols = np.ones(L, bool) if keep is None else keep
    wrong_order = kcols & (is_n.sum(axis=0) <= math.floor(F * n))
    assert not wrong_order[SPECIAL].any()
    assert not np.array_equal(e["kept_sites"], kcols)                                                   # the N share drops columns too
    return e
