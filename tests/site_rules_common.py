"""Shared by the site-rule tests: the standard input, the standard rule, and "is N" taken from the library's own letter table."""
import math

import numpy as np

SIZES = [(70, 5000), (131, 30001), (700, 9000)]


def is_n_table(hiplib):
    """bool[256]: the bytes the pack stores as N (tracs_debug_iupac_mask == 15), not a list of letters"""
    return np.array([hiplib.tracs_debug_iupac_mask(ch) == 15 for ch in range(256)], bool)


def run_columns(L):
    """three runs of L // 40 columns"""
    out = np.zeros(L, bool)
    for k in (1, 2, 3):
        s = k * (L // 4) + 7
        out[s:s + L // 40] = True
    return out


def standard_input(n, L, seed=11):
    """synth.alignment + three runs of L / 40 columns in which every sample becomes N with p = 0.4 -> (seqs, run columns)"""
    from tracs_amd import synth
    seqs = synth.alignment(n, L, seed, mu_lineage=3e-3, mu_sample=1e-3, p_n=0.02, p_partial=0.005)
    runs = run_columns(L)
    rng = np.random.default_rng(seed + 1000)
    hit = rng.random((n, int(runs.sum()))) < 0.4
    block = seqs[:, runs]
    block[hit] = ord("N")
    seqs[:, runs] = block
    return seqs, runs


def standard_files_keep(L):
    """the file part of the standard rule: a mask of [100, 357), the last 200 columns and column 0 -> bool[L], True = may stay"""
    keep = np.ones(L, bool)
    keep[100:357] = False
    keep[L - 200:] = False
    keep[0] = False
    return keep


def standard_rule(seqs, isn):
    """-> (keep bool[L] of the files, max_n_samples = floor(0.2 n), kept bool[L] computed in numpy)"""
    n, L = seqs.shape
    keep = standard_files_keep(L)
    max_n = math.floor(0.2 * n)
    kept = keep & (isn[seqs].sum(axis=0) <= max_n)
    return keep, max_n, kept
