"""`tracs distance --mst WEIGHT` on the host: the flag, its refusals before any GPU call, and the CPU forest helper (tests/forest_ref.py)
against connected components of the whole weighted graph at every threshold."""
import argparse
import os

import numpy as np
import pytest

import forest_ref as fr


def _parser():
    from tracs_amd.distance import distance_parser
    return distance_parser(argparse.ArgumentParser())


def test_mst_default_off():
    assert _parser().parse_args(["--msa", "x.fa", "-o", "o.csv"]).mst is None


@pytest.mark.parametrize("w", ["snp", "filter", "direct", "expectedK"])
def test_mst_accepts_the_cluster_weights(w):
    assert _parser().parse_args(["--msa", "x.fa", "-o", "o.csv", "--mst", w]).mst == w


def test_mst_rejects_other_words(capsys):
    with pytest.raises(SystemExit) as e:
        _parser().parse_args(["--msa", "x.fa", "-o", "o.csv", "--mst", "hamming"])
    assert e.value.code == 2
    assert "argument --mst" in capsys.readouterr().err


@pytest.mark.parametrize("extra,words", [
    (["--mst", "snp", "--nearest", "3"], ["--mst", "--nearest"]),
    (["--mst", "snp", "--gpus", "2"], ["--mst", "--gpus 1"]),
    (["--mst", "filter"], ["--mst filter", "--filter"]),
    (["--mst", "direct"], ["--mst direct", "--meta"]),
    (["--mst", "expectedK", "--filter"], ["--mst expectedK", "--meta"]),
])
def test_mst_refusals_before_the_gpu(tmp_path, monkeypatch, extra, words):
    import tracs_amd.distance as di
    from tracs_amd import _lib, multigpu

    def no_gpu(*a, **k):
        raise AssertionError("the GPU library or a GPU path was entered")
    for mod, name in ((multigpu, "spawn"), (multigpu, "init"), (_lib, "load"), (_lib, "require_gpu"), (di, "nearest_arrays"),
                      (di, "pairsnp_arrays")):
        monkeypatch.setattr(mod, name, no_gpu)
    out = tmp_path / "o.csv"
    a = _parser().parse_args(["--msa", "x.fa", "-o", str(out)] + extra)
    with pytest.raises(SystemExit) as e:
        a.func(a)
    msg = str(e.value.code)
    assert e.value.code not in (0, None)
    for w in words:
        assert w in msg, (w, msg)
    assert not os.path.exists(out)


def _check_helper(n, i, j, w):
    """The helper's forest joins, at every threshold, exactly the samples that all edges up to it join."""
    f = fr.forest(n, i, j, w)
    assert len(f) <= max(n - 1, 0) and len(set(f.tolist())) == len(f)
    wf = np.asarray(w, np.float64)
    vals = np.unique(wf[~np.isnan(wf)])
    ts = sorted(set(vals.tolist()) | {-np.inf, np.inf, float(vals.min()) - 1 if len(vals) else 0.0}
                | {float((a + b) / 2) for a, b in zip(vals[:-1], vals[1:])})
    for t in ts:
        got = fr.threshold_partition(n, np.asarray(i)[f], np.asarray(j)[f], wf[f], t)
        exp = fr.threshold_partition(n, i, j, wf, t)
        assert got == exp, t
    # the sample set and the whole-graph components (NaN edges included)
    assert fr.partition(n, np.asarray(i)[f], np.asarray(j)[f]) == fr.partition(n, i, j)
    return f


def _random_graph(rng, n, m, isolated=0):
    pairs = set()
    live = n - isolated
    while len(pairs) < m:
        a, b = rng.integers(0, live, 2)
        if a != b:
            pairs.add((int(min(a, b)), int(max(a, b))))
    p = np.array(sorted(pairs), np.int64).reshape(-1, 2)
    flip = rng.random(len(p)) < 0.5                       # either orientation
    return np.where(flip, p[:, 1], p[:, 0]), np.where(flip, p[:, 0], p[:, 1])


@pytest.mark.parametrize("seed", range(4))
def test_helper_heavy_ties(seed):
    rng = np.random.default_rng(seed)
    n = 60
    i, j = _random_graph(rng, n, 150, isolated=7)
    _check_helper(n, i, j, rng.integers(0, 4, len(i)))


def test_helper_u32_weights():
    rng = np.random.default_rng(7)
    n = 80
    i, j = _random_graph(rng, n, 400)
    _check_helper(n, i, j, rng.integers(0, 2 ** 32, len(i), dtype=np.uint64))


@pytest.mark.parametrize("seed", range(3))
def test_helper_f64_special_values(seed):
    rng = np.random.default_rng(100 + seed)
    n = 70
    i, j = _random_graph(rng, n, 300, isolated=5)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-300, -1e-300, 0.5, 2.0, 0.5])
    w = np.where(rng.random(len(i)) < 0.6, pool[rng.integers(0, len(pool), len(i))], rng.normal(size=len(i)))
    f = _check_helper(n, i, j, w)
    # -0.0 ties +0.0: the order falls through to (i, j)
    o = fr.order(np.array([0, 0]), np.array([2, 1]), np.array([-0.0, 0.0]))
    assert o.tolist() == [1, 0]
    assert len(f) == n - 5 - len(fr.partition(n, i, j))


def test_helper_nan_edges_keep_their_samples():
    i, j = np.array([0, 1, 2]), np.array([1, 2, 3])
    w = np.array([np.nan, 1.0, np.nan])
    f = fr.forest(4, i, j, w)
    assert f.tolist() == [0, 1, 2]                        # a NaN row is the only one naming samples 0 and 3


def test_helper_bipartite():
    rng = np.random.default_rng(3)
    n0, n1 = 15, 40
    pairs = [(a, n0 + b) for a in range(n0) for b in range(n1) if rng.random() < 0.3]
    i = np.array([p[0] for p in pairs])
    j = np.array([p[1] for p in pairs])
    f = _check_helper(n0 + n1, i, j, rng.integers(0, 5, len(i)))
    assert (i[f] < n0).all() and (j[f] >= n0).all()


def test_helper_forest_of_a_forest_is_itself():
    """The cycle property the device update relies on: MSF(MSF(A) u B) == MSF(A u B)."""
    rng = np.random.default_rng(11)
    n = 90
    i, j = _random_graph(rng, n, 700)
    w = rng.integers(0, 6, len(i))
    whole = fr.forest(n, i, j, w)
    a = np.arange(len(i)) < 350
    fa = np.flatnonzero(a)[fr.forest(n, i[a], j[a], w[a])]
    rest = np.concatenate([fa, np.flatnonzero(~a)])
    again = rest[fr.forest(n, i[rest], j[rest], w[rest])]
    key = lambda s: sorted((int(min(i[e], j[e])), int(max(i[e], j[e]))) for e in s)
    assert key(again) == key(whole)
