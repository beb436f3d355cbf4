"""BIONJ on the host: the definition restated in tests/bionj_ref.py against itself -- the running-sum lambda against
Gascuel's explicit sum in exact rationals, float64 against rationals on split sets, tree metrics, the matrix on which BIONJ is not
neighbour joining, degenerate inputs -- and `--tree bionj` through the parser, the refusals, the request and the handle, all
without a GPU."""
import argparse
import ctypes as C
import contextlib
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import bionj_ref
import nj_ref
from test_tree_cli import REFUSALS, _no_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, seed) of bionj_ref.noisy_tree_metric: eight per n = 5 .. 12.  The rational run of every one has no exact Q tie above r = 4 (the
# test asserts it); (8, 8003) and (11, 11001) have one and are replaced by the next free seed of their n.
EXACT_CASES = [(n, 1000 * n + s) for n in range(5, 13) for s in range(8) if (n, s) not in ((8, 3), (11, 1))] + [(8, 8008), (11, 11008)]


def _parser():
    from tracs_amd.distance import distance_parser
    return distance_parser(argparse.ArgumentParser())


def float_splits(D):
    return set(nj_ref.splits_of(D.shape[0], *bionj_ref.bionj(D)))


def patristic(n, parent, child, length):
    """leaf-to-leaf path lengths of a tree given as edges in creation order"""
    nodes = int(max(parent.max(), child.max())) + 1
    adj = [[] for _ in range(nodes)]
    for p, c, x in zip(parent.tolist(), child.tolist(), length.tolist()):
        adj[p].append((c, x)); adj[c].append((p, x))
    P = np.zeros((n, n))
    for s in range(n):
        dist, stack = {s: 0.0}, [s]
        while stack:
            u = stack.pop()
            for v, x in adj[u]:
                if v not in dist:
                    dist[v] = dist[u] + x
                    stack.append(v)
        P[s] = [dist[k] for k in range(n)]
    return P


def test_running_sum_lambda_is_gascuels_and_the_sums_are_the_row_sums():
    seen = []

    def check(r, lam, explicit, R, RV, M, W):
        assert lam == explicit, (r, lam, explicit)
        assert R == [sum(row) for row in M] and RV == [sum(row) for row in W], r
        assert all(M[k][k] == 0 and W[k][k] == 0 for k in range(r)) and all(M[p][q] == M[q][p] and W[p][q] == W[q][p] for p in range(r) for q in range(p))
        seen.append(lam)
    for n, seed in EXACT_CASES[::4] + [(6, None)]:
        D = bionj_ref.NJ_DIFFERS if seed is None else bionj_ref.noisy_tree_metric(n, seed)
        joins, edges, _ = bionj_ref.bionj_exact(D, check)
        assert len(joins) == n - 3 and len(edges) == 2 * n - 3
    lams = [x for x in seen if x is not None]
    assert any(x not in (Fraction(0), Fraction(1, 2), Fraction(1)) for x in lams)           # (the weights are exercised)
    assert any(x.denominator & (x.denominator - 1) for x in lams)                           # (and not dyadic: float64 must round them)


@pytest.mark.parametrize("n", [4, 5, 8, 33, 120])
def test_a_tree_metric_comes_back_with_every_split(n):
    D, want = nj_ref.random_tree_metric(n, np.random.default_rng(100 + n))
    parent, child, length = bionj_ref.bionj(D)
    got = nj_ref.splits_of(n, parent, child, length)
    assert set(got) == set(want)
    tol = 1e-9 * D.max()
    assert max(abs(got[s] - want[s]) for s in want) <= tol
    assert np.abs(patristic(n, parent, child, length) - D).max() <= 2 * n * tol


@pytest.mark.parametrize("n,seed", EXACT_CASES, ids=["%d-%d" % c for c in EXACT_CASES])
def test_float64_and_rationals_give_the_same_splits(n, seed):
    """split sets, not records: at r = 4 the two complementary pairs tie exactly for every input and rounding picks one"""
    D = bionj_ref.noisy_tree_metric(n, seed)
    joins, edges, ties = bionj_ref.bionj_exact(D)
    assert [r for r, tied in ties if tied and r > 4] == [], "the case has an exact Q tie above r = 4: choose another seed"
    assert (4, True) in ties
    assert float_splits(D) == bionj_ref.exact_splits(n, edges)


def test_bionj_is_not_neighbour_joining():
    D = bionj_ref.NJ_DIFFERS
    assert np.array_equal(D, D.T) and not D.diagonal().any()
    s_nj = set(nj_ref.splits_of(6, *nj_ref.nj(D)))
    s_bio = float_splits(D)
    assert s_nj != s_bio and len(s_nj) == len(s_bio) == 9
    assert s_nj == set(nj_ref.splits_of(6, *[np.array(x) for x in zip(*[(p, c, float(x)) for p, c, x in nj_ref.nj_exact(D)[1]])]))
    assert s_bio == bionj_ref.exact_splits(6, bionj_ref.bionj_exact(D)[1])                  # (both in exact arithmetic as well)


def test_the_zero_matrix_and_small_n_are_neighbour_joinings():
    for D in [np.zeros((n, n)) for n in (0, 1, 2, 3, 4, 9)] + [7.0 * (np.ones((n, n)) - np.eye(n)) for n in (1, 2, 3)]:
        got, want = bionj_ref.bionj_records(D), nj_ref.nj_records(D)
        for g, w in zip(list(got[0]) + list(got[1:]), list(want[0]) + list(want[1:])):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), D.shape
    trace = []
    bionj_ref.bionj_records(np.zeros((9, 9)), trace)
    assert trace == [(0.5, 0.0, 0.5)] * 6


def test_duplicated_samples_take_the_half_weight():
    n = 12
    D = bionj_ref.noisy_tree_metric(n, 77)
    D[n - 1] = D[2]; D[:, n - 1] = D[:, 2]                  # sample n - 1 is sample 2 again, and 7 is 5 again
    D[7] = D[5]; D[:, 7] = D[:, 5]
    np.fill_diagonal(D, 0.0)
    D[2, n - 1] = D[n - 1, 2] = D[5, 7] = D[7, 5] = 0.0
    assert np.array_equal(D, D.T)
    trace = []
    rec, ids, d = bionj_ref.bionj_records(D, trace)
    zero = [k for k, (lam, v, raw) in enumerate(trace) if v == 0.0]
    assert sorted((int(rec[0][k]), int(rec[1][k])) for k in zero) == [(2, n - 1), (5, 7)] and all(trace[k][0] == 0.5 for k in zero)
    parent, child, length = nj_ref.nj_edges(n, rec, ids, d)
    assert np.isfinite(length).all()
    P = patristic(n, parent, child, length)
    assert abs(P[2, n - 1]) <= 1e-9 * D.max() and abs(P[5, 7]) <= 1e-9 * D.max()


def test_lambda_is_clamped_at_both_ends():
    """seeded 6 x 6 integer matrices far from a tree: the unclamped weight leaves [0, 1] on either side"""
    low = high = 0
    for seed in (0, 1, 5, 8, 11):
        U = np.triu(np.random.default_rng(seed).integers(1, 60, (6, 6)), 1)
        trace = []
        rec, ids, d = bionj_ref.bionj_records((U + U.T).astype(np.float64), trace)
        for lam, v, raw in trace:
            assert 0.0 <= lam <= 1.0 and (lam == raw or (raw < 0.0 and lam == 0.0) or (raw > 1.0 and lam == 1.0))
            low += raw < 0.0
            high += raw > 1.0
        assert np.isfinite(nj_ref.nj_edges(6, rec, ids, d)[2]).all()
    assert low >= 2 and high >= 2


# ---- the command line, the request, the handle ------------------------------------------------------------------------------------

def test_the_parser_takes_bionj_and_nothing_else_new(capsys):
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "bionj", "--tree-distance", "per-site", "--tree-edges", "e.csv"])
    assert (a.tree, a.tree_distance, a.tree_edges) == ("bionj", "per-site", "e.csv")
    assert _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj"]).tree == "nj"
    with pytest.raises(SystemExit):
        _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "upgma"])
    with pytest.raises(SystemExit):
        _parser().parse_args(["-h"])
    text = " ".join(capsys.readouterr().out.split()).replace("- ", "-")
    for words in ("bionj: the BIONJ tree (Gascuel 1997)", "minimise the variance of the new row", "about twice its memory"):
        assert words in text, words


BIONJ_REFUSALS = [([("bionj" if x == "nj" else x) for x in extra], words) for extra, words in REFUSALS]


@pytest.mark.parametrize("extra,words", BIONJ_REFUSALS, ids=[" ".join(r[0]) for r in BIONJ_REFUSALS])
def test_every_refusal_of_the_tree_holds_for_bionj(tmp_path, monkeypatch, extra, words):
    _no_gpu(monkeypatch)
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "o.nwk"
    a = _parser().parse_args(["--msa", "x.fa", "-o", str(out)] + extra)
    with pytest.raises(SystemExit) as e:
        a.func(a)
    msg = str(e.value.code)
    assert msg.startswith("tracs distance: ") and "\n" not in msg
    for w in words:
        assert w in msg, (w, msg)
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "e.csv")


def test_bootstrap_takes_no_per_site_distance_with_bionj_either(tmp_path, monkeypatch):
    _no_gpu(monkeypatch)
    a = _parser().parse_args(["--msa", "x.fa", "-o", str(tmp_path / "o.nwk"), "--tree", "bionj", "--tree-distance", "per-site", "--bootstrap", "4"])
    with pytest.raises(SystemExit) as e:
        a.func(a)
    assert "--tree-distance per-site" in str(e.value.code)


def test_the_request_mirrors_still_match_the_header(tmp_path):
    from tracs_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    src, exe = tmp_path / "k.c", tmp_path / "k"
    src.write_text('#include <stdio.h>\n#include "tracs_hip.h"\nint main(void)\n{\n    printf("%d %zu %zu %zu\\n", TRACS_TREE_BIONJ, '
                   'sizeof(tracs_tree_request), offsetof(tracs_tree_request, kind), offsetof(tracs_tree_request, create));\n    return 0;\n}\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert got == [str(_lib.TREE_BIONJ), str(C.sizeof(_lib.TreeRequest)), str(_lib.TreeRequest.kind.offset), str(_lib.TreeRequest.create.offset)]
    assert _lib.TREE_BIONJ == 2 and len(_lib.TreeRequest._fields_) == 19 and len(_lib.TreeResult._fields_) == 6


def test_the_library_has_the_bionj_entries(hiplib):
    from tracs_amd import _lib
    header = open(os.path.join(ROOT, "include", "tracs_hip.h")).read()
    assert re.search(r"^size_t tracs_bionj_state_bytes\(size_t n\);", header, re.M) and re.search(r"^int tracs_bionj_run\(", header, re.M)
    for name in ("tracs_bionj_state_bytes", "tracs_bionj_run"):
        assert hasattr(hiplib, name) and name in _lib.SYMBOLS, name
    n = 10000
    assert 2 * 8 * n * n <= hiplib.tracs_bionj_state_bytes(n) < 2 * 8 * n * n + (1 << 20)
    assert hiplib.tracs_bionj_state_bytes(n) - hiplib.tracs_nj_state_bytes(n) <= 8 * n * n + 3 * 8 * n + 4 * 256     # (V, RV, two rows)
    assert hiplib.tracs_bionj_state_bytes(0) > hiplib.tracs_nj_state_bytes(0) > 0
    assert hiplib.tracs_bionj_state_bytes(2 ** 24) > 0 and hiplib.tracs_bionj_state_bytes(2 ** 24 + 1) == 0
    assert hiplib.tracs_bionj_run(None, 10, None) == -1 and hiplib.tracs_last_error().startswith(b"tracs_bionj_run: NULL state")
    assert hiplib.tracs_nj_run(None, 10, None) == -1 and hiplib.tracs_last_error().startswith(b"tracs_nj_run: NULL state")
    blob = open(_lib.LIB_PATH, "rb").read()
    for kernel in (b"bionj_rows_kernel", b"nj_rows_kernel", b"nj_scan_kernel", b"nj_commit_kernel"):
        assert kernel in blob, kernel


def test_the_handle_puts_the_method_into_kind():
    from tracs_amd.handle import DistanceHandle
    kinds = []

    class Lib:
        def tracs_distance_tree_run(self, h, req, res):
            kinds.append(("run", req._obj.kind, req._obj.replicates))
            return 0

        def tracs_distance_tree_iterate(self, h, req, it, res, ires):
            kinds.append(("iterate", req._obj.kind, it._obj.max_iterations))
            return 0
    h = DistanceHandle.__new__(DistanceHandle)
    h.L, h.h = Lib(), None
    h.tree("o", "r")
    h.tree("o", "r", method="nj", per_site=True)
    h.tree("o", "r", method="bionj")
    h.tree("o", "r", method="bionj", per_site=True, edges_path="e")
    h.tree("o", "r", method="bionj", bootstrap=8, seed=3)
    h.tree("o", "r", method="bionj", edges_path="e", tree_filter=True, iterate=3)
    assert kinds == [("run", 0, 0), ("run", 1, 0), ("run", 2, 0), ("run", 3, 0), ("run", 2, 8), ("iterate", 2, 3)]
    with pytest.raises(ValueError, match="method is 'nj' or 'bionj'"):
        h.tree("o", "r", method="upgma")
    with pytest.raises(ValueError, match="SNP distance only"):
        h.tree("o", "r", method="bionj", per_site=True, bootstrap=4)
    assert len(kinds) == 6


def test_the_command_hands_the_method_to_the_handle_and_names_it(monkeypatch):
    import tracs_amd.distance as di
    from tracs_amd.handle import TreeResult
    calls = []

    class Handle:
        def tree(self, *a, **kw):
            calls.append(kw)
            return TreeResult(7, 17, 0, 0, 0, 0)

    @contextlib.contextmanager
    def opened(*a, **kw):
        yield Handle()
    monkeypatch.setattr(di, "_opened", opened)
    lines = {}
    for method in ("nj", "bionj"):
        args = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", method, "--tree-edges", "e.csv"])
        args.tree_files_made = False
        seen = []
        di._tree_on_device(["x.fa"], args, None, "x", seen.append)
        lines[method] = seen
    assert "method" not in calls[0] and calls[1]["method"] == "bionj"
    assert lines["nj"] == ["[sum] tracs_distance_tree (dense panels, joins, tree: 7 joins, 17 edge rows written)"]
    assert lines["bionj"] == [lines["nj"][0] + " [bionj]"]
