"""`tracs distance --ancestors WEIGHT` on the host: the flags, their refusals before any GPU call, and the CPU helper
(tests/ancestors_ref.py) against an O(n^2) brute force written from the definition's words."""
import argparse
import os

import numpy as np
import pytest

import ancestors_ref as ar


def _parser():
    from tracs_amd.distance import distance_parser
    return distance_parser(argparse.ArgumentParser())


def test_ancestors_default_off():
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.csv"])
    assert a.ancestors is None and a.ancestors_out is None


@pytest.mark.parametrize("w", ["snp", "filter", "direct", "expectedK"])
def test_ancestors_accepts_the_four_weights(w):
    assert _parser().parse_args(["--msa", "x.fa", "-o", "o.csv", "--ancestors", w]).ancestors == w


def test_ancestors_rejects_other_words(capsys):
    with pytest.raises(SystemExit) as e:
        _parser().parse_args(["--msa", "x.fa", "-o", "o.csv", "--ancestors", "hamming"])
    assert e.value.code == 2
    assert "argument --ancestors" in capsys.readouterr().err


def test_help_states_the_direction_of_direct_and_the_trees():
    text = " ".join(_parser().format_help().split()).replace("- ", "-")        # (argparse may wrap at a hyphen)
    assert "LARGEST first" in text and "--mst direct" in text
    assert "transmission trees" in text and "not single-linkage clusters" in text


META = ["--meta", "dates.csv"]


@pytest.mark.parametrize("extra,words", [
    (["--ancestors", "snp"], ["--ancestors snp", "--meta"]),
    (["--ancestors", "filter", "--filter"], ["--ancestors filter", "--meta"]),
    (["--ancestors", "direct"], ["--ancestors direct", "--meta"]),
    (["--ancestors", "expectedK"], ["--ancestors expectedK", "--meta"]),
    (["--ancestors", "filter"] + META, ["--ancestors filter", "--filter"]),
    (["--ancestors", "snp", "--msa-db", "db.fa"] + META, ["--ancestors", "--msa-db"]),
    (["--ancestors", "snp", "--gpus", "2"] + META, ["--ancestors", "--gpus 1"]),
    (["--ancestors", "snp", "--gpus", "8"] + META, ["--ancestors", "--gpus 1"]),
    (["--ancestors", "snp", "--mst", "snp"] + META, ["--ancestors", "--mst"]),
    (["--ancestors", "snp", "--nearest", "3"] + META, ["--ancestors", "--nearest"]),
    (["--ancestors", "snp", "--histogram"], ["--ancestors", "--histogram"]),
    (["--ancestors", "snp", "--histogram"] + META, ["--ancestors", "--histogram"]),
    (["--ancestors-out", "tree.csv"] + META, ["--ancestors-out", "--ancestors"]),
    (["--ancestors-out", "tree.csv", "--mst", "snp"], ["--ancestors-out", "--ancestors"]),
])
def test_ancestors_refusals_before_the_gpu(tmp_path, monkeypatch, extra, words):
    import tracs_amd.distance as di
    from tracs_amd import _lib, multigpu

    def no_gpu(*a, **k):
        raise AssertionError("the GPU library or a GPU path was entered")
    for mod, name in ((multigpu, "spawn"), (multigpu, "init"), (_lib, "load"), (_lib, "require_gpu"), (di, "nearest_arrays"),
                      (di, "pairsnp_arrays")):
        monkeypatch.setattr(mod, name, no_gpu)
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "o.csv"
    a = _parser().parse_args(["--msa", "x.fa", "-o", str(out)] + extra)
    with pytest.raises(SystemExit) as e:
        a.func(a)
    msg = str(e.value.code)
    assert e.value.code not in (0, None)
    for w in words:
        assert w in msg, (w, msg)
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "tree.csv")


def test_check_ancestors_args_passes_a_complete_command():
    from tracs_amd.distance import check_ancestors_args
    for extra in (["--ancestors", "snp"], ["--ancestors", "filter", "--filter"], ["--ancestors", "direct", "--ancestors-out", "t.csv"],
                  ["--ancestors", "expectedK", "-K", "3", "-D", "10", "--min-sites", "5", "--max-sample-n-share", "0.5"], []):
        check_ancestors_args(_parser().parse_args(["--msa", "x.fa", "-o", "o.csv"] + META + extra))


# ---- the helper against the brute force ---------------------------------------------------------------------------------------

def _graph(rng, n, m):
    pairs = set()
    while len(pairs) < m:
        a, b = rng.integers(0, n, 2)
        if a != b:
            pairs.add((int(min(a, b)), int(max(a, b))))
    p = np.array(sorted(pairs), np.int64).reshape(-1, 2)
    rng.shuffle(p)
    flip = rng.random(len(p)) < 0.5                       # either orientation
    return np.where(flip, p[:, 1], p[:, 0]), np.where(flip, p[:, 0], p[:, 1])


POOL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-300, 0.25, 0.25, 3.0])


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_helper_against_brute_force(seed, kind):
    """Few distinct values, days and gaps: ties in the value, then in the gap, are settled by the index."""
    rng = np.random.default_rng(seed * 3 + kind)
    n = 40
    i, j = _graph(rng, n, 200)
    days = rng.integers(-3, 3, n) * 2                     # a small pool with negative days: equal days and equal gaps are common
    v = rng.integers(0, 3, len(i)) if kind == 0 else np.where(rng.random(len(i)) < 0.7, POOL[rng.integers(0, len(POOL), len(i))],
                                                              rng.integers(0, 2, len(i)) * 0.5)
    elig = rng.random(len(i)) < 0.8 if seed % 2 else None
    p, e = ar.ancestors(n, days, i, j, v, kind, elig)
    bp, be = ar.brute_force(n, days, i, j, v, kind, elig)
    assert np.array_equal(p, bp) and np.array_equal(e, be)
    linked = p >= 0
    assert (days[p[linked]] < days[linked]).all() and linked.sum() < n
    chosen = e[linked]
    assert len(set(chosen.tolist())) == len(chosen)       # a pair is chosen by its later sample only
    root, gen = ar.trees(p)
    assert (gen[~linked] == 0).all() and np.array_equal(root[~linked], np.flatnonzero(~linked))
    assert np.array_equal(gen[linked], gen[p[linked]] + 1) and np.array_equal(root[linked], root[p[linked]])


def test_helper_key_parts_by_hand():
    days = np.array([0, 0, 5, 3, -4])
    # sample 2 (day 5): candidates 0 (value 1, gap 5), 1 (value 1, gap 5), 3 (value 1, gap 2), 4 (value 0, gap 9)
    i, j = np.array([2, 1, 3, 4, 0]), np.array([0, 2, 2, 2, 1])
    p, e = ar.ancestors(5, days, i, j, np.array([1, 1, 1, 0, 0]), 0)
    assert p[2] == 4 and e[2] == 3                        # the value decides first
    p, e = ar.ancestors(5, days, i, j, np.array([1, 1, 1, 1, 0]), 0)
    assert p[2] == 3 and e[2] == 2                        # then the smaller gap
    p, e = ar.ancestors(5, days, i[[0, 1, 4]], j[[0, 1, 4]], np.array([1, 1, 0]), 0)
    assert p[2] == 0 and e[2] == 0                        # then the index
    assert p[0] == -1 and p[1] == -1                      # the same-day pair {0, 1} links nobody
    # descending with the zeros tied, NaN last, -inf before it
    v = np.array([-0.0, 0.0, -np.inf, np.nan, 7.0])
    p, _ = ar.ancestors(5, days, i, j, v, 2)
    assert p[2] == 0                                      # -0.0 ties +0.0, equal gap: index 0 before index 1
    p, _ = ar.ancestors(5, days, i[2:4], j[2:4], v[2:4], 2)
    assert p[2] == 3                                      # -inf before NaN
    p, _ = ar.ancestors(5, days, i[2:4], j[2:4], v[2:4], 1)
    assert p[2] == 3                                      # ascending: -inf first as well


def test_trees_chain_and_star():
    n = 3000
    p = np.arange(-1, n - 1)
    root, gen = ar.trees(p)
    assert (root == 0).all() and np.array_equal(gen, np.arange(n))
    p = np.zeros(50, np.int64)
    p[0] = -1
    root, gen = ar.trees(p)
    assert (root == 0).all() and gen[0] == 0 and (gen[1:] == 1).all()
