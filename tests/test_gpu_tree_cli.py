"""`tracs distance --tree nj` end to end (tracs_distance_tree): the Newick line and the edges file against the definition
(tests/nj_ref.py) on the oracle's distances.  Topology and lengths are compared exactly, lengths as doubles."""
import argparse
import math
import os

import numpy as np
import pytest

import nj_ref
from site_rules_common import is_n_table

pytestmark = pytest.mark.gpu


def run_cli(argv):
    from tracs_amd.distance import distance_parser
    a = distance_parser(argparse.ArgumentParser()).parse_args(argv + ["--loglevel", "ERROR"])
    a.func(a)


def write(path, seqs, names=None):
    from tracs_amd import synth
    return synth.write_fasta(str(path), seqs, names=names or ["s%d" % i for i in range(seqs.shape[0])], width=60)


def oracle_matrices(O, seqs):
    n = seqs.shape[0]
    D, N = np.zeros((n, n)), np.zeros((n, n))
    if n >= 2:
        r, c, d, nn = O.pairsnp_arrays(seqs, n_threads=8)
        D[r.astype(np.int64), c.astype(np.int64)] = d
        N[r.astype(np.int64), c.astype(np.int64)] = nn
    return D + D.T, N + N.T


def expected_edges(O, seqs, per_site=False):
    D, N = oracle_matrices(O, seqs)
    if per_site:
        iu = np.triu_indices(seqs.shape[0], 1)
        Q = np.zeros_like(D)
        Q[iu] = D[iu] / N[iu]
        D = Q + Q.T
    return nj_ref.nj(D)


def check_tree(line, names, edges):
    """one Newick line describes exactly the tree of `edges` = (parent, child, length) over the leaves `names`"""
    n = len(names)
    nodes = nj_ref.parse_newick(line)
    got = nj_ref.newick_splits(nodes, names)                            # (asserts that the leaves are the names)
    want = nj_ref.splits_of(n, *edges)
    assert got.keys() == want.keys()
    assert got == want, [(k, got[k], want[k]) for k in got if got[k] != want[k]][:5]
    assert sum(1 for p, lab, _ in nodes if lab is None) == n - 2 and nodes[0] == (None, None, None)      # binary, unlabelled inner nodes


def check_edge_rows(rows, names, edges, ref):
    """the rows of --tree-edges are the edges in creation order, internal node n + t as #<t + 1>"""
    n = len(names)
    name = lambda v: names[v] if v < n else "#%d" % (v - n + 1)        # noqa: E731
    parent, child, length = edges
    assert len(rows) == len(parent) == 2 * n - 3
    for row, p, c, x in zip(rows, parent.tolist(), child.tolist(), length.tolist()):
        f = row.rsplit(",", 2)
        assert f[0] == name(p) + "," + name(c) and float(f[1]) == x and f[2] == ref, (row, p, c, x)


@pytest.fixture(scope="module")
def base():
    from tracs_amd import synth
    return synth.alignment(65, 3000, seed=31, mu_lineage=5e-3, mu_sample=2e-3, p_n=0.03, p_partial=0.01, p_lower=0.02)


def test_tree_and_edges_of_one_alignment(hiplib, oracle, base, tmp_path):
    fa, out, ed = tmp_path / "ref1_combined.fasta", tmp_path / "t.nwk", tmp_path / "e.csv"
    names = write(fa, base)
    run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(out), "--tree-edges", str(ed)])
    lines = out.read_text().split("\n")
    assert len(lines) == 2 and lines[1] == "" and lines[0].endswith(";")
    edges = expected_edges(oracle, base)
    check_tree(lines[0], names, edges)
    rows = ed.read_text().split("\n")
    assert rows[0] == "parent,child,length,MSA file" and rows[-1] == ""
    check_edge_rows(rows[1:-1], names, edges, "ref1")
    # the Python entry point on the same matrix: the same edges
    from tracs_amd import api
    D, _ = oracle_matrices(oracle, base)
    got = api.neighbor_joining(D)
    for g, w in zip(got, edges):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    import torch
    got = api.neighbor_joining(torch.from_numpy(D).cuda())
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, edges))
    for bad, word in ((-D, "negative"), (D + np.eye(65), "diagonal"), (np.triu(D), "symmetric"), (D * np.inf, "non-finite"), (D[:3], "square")):
        with pytest.raises(ValueError, match=word):
            api.neighbor_joining(bad)


@pytest.mark.parametrize("rows", ["1", "7", "64"])
def test_panels_smaller_than_the_alignment(hiplib, oracle, base, tmp_path, monkeypatch, rows):
    """TRACS_FOREST_PANEL_ROWS: the panel walk of tracs_distance_tree crosses panel boundaries (shifted panel bases, several loads)"""
    monkeypatch.setenv("TRACS_FOREST_PANEL_ROWS", rows)
    fa, out, ed = tmp_path / "a.fa", tmp_path / "t.nwk", tmp_path / "e.csv"
    names = write(fa, base)
    run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(out), "--tree-edges", str(ed)])
    edges = expected_edges(oracle, base)
    check_tree(out.read_text(), names, edges)
    check_edge_rows(ed.read_text().split("\n")[1:-1], names, edges, "a")
    run_cli(["--msa", str(fa), "--tree", "nj", "--tree-distance", "per-site", "-o", str(out)])
    check_tree(out.read_text(), names, expected_edges(oracle, base, per_site=True))


def test_per_site_distances(hiplib, oracle, base, tmp_path):
    fa, out = tmp_path / "a.fa", tmp_path / "t.nwk"
    names = write(fa, base)
    run_cli(["--msa", str(fa), "--tree", "nj", "--tree-distance", "per-site", "-o", str(out)])
    check_tree(out.read_text(), names, expected_edges(oracle, base, per_site=True))
    # two samples that share no known site: refused by name, pointing at the sample rule
    seqs = base[:6].copy()
    seqs[1, :1500] = ord("N")
    seqs[4, 1500:] = ord("-")
    write(fa, seqs)
    with pytest.raises(RuntimeError, match=r"'s1' and 's4'.*--max-sample-n-share"):
        run_cli(["--msa", str(fa), "--tree", "nj", "--tree-distance", "per-site", "-o", str(out)])
    run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(out)])          # SNP distances do not need one
    check_tree(out.read_text(), names[:6], expected_edges(oracle, seqs))


def test_two_alignments_give_two_lines(hiplib, oracle, base, tmp_path):
    fa, fb, out, ed = tmp_path / "one.fa", tmp_path / "two_combined.fa", tmp_path / "t.nwk", tmp_path / "e.csv"
    sa, sb = base[:40], base[20:][::-1].copy()
    na, nb = write(fa, sa), write(fb, sb, names=["q%d" % i for i in range(sb.shape[0])])
    run_cli(["--msa", str(fa), str(fb), "--tree", "nj", "-o", str(out), "--tree-edges", str(ed)])
    lines = out.read_text().split("\n")
    assert len(lines) == 3 and lines[2] == ""
    ea, eb = expected_edges(oracle, sa), expected_edges(oracle, sb)
    check_tree(lines[0], na, ea)
    check_tree(lines[1], nb, eb)
    rows = ed.read_text().split("\n")[1:-1]
    check_edge_rows(rows[:2 * 40 - 3], na, ea, "one")
    check_edge_rows(rows[2 * 40 - 3:], nb, eb, "two")


def test_rules_give_the_tree_of_the_reduced_alignment(hiplib, oracle, base, tmp_path):
    """--mask / --max-n-share and --max-sample-n-share: the tree of the FASTA with those columns / records deleted"""
    isn = is_n_table(hiplib)
    seqs = base.copy()
    n, L = seqs.shape
    rng = np.random.default_rng(2)
    for s in (0, 17, 64):                                              # three records that are mostly N
        seqs[s, rng.random(L) < 0.6] = ord("N")
    cols = rng.choice(L, 150, replace=False)
    for c in cols:                                                      # columns at which a third of the samples is N
        seqs[rng.random(n) < 0.35, c] = ord("N")
    G, F = 0.3, 0.2
    mask = np.zeros(L, bool)
    mask[50:400] = True
    mask[L - 100:] = True
    file_keep = ~mask
    counts = isn[seqs][:, file_keep].sum(axis=1)
    kept_samples = counts <= math.floor(G * int(file_keep.sum()))
    kept_sites = file_keep & (isn[seqs][kept_samples].sum(axis=0) <= math.floor(F * int(kept_samples.sum())))
    assert (~kept_samples).sum() == 3 and 50 < (file_keep & ~kept_sites).sum() < 400
    fa, bed, out, out2 = tmp_path / "full.fa", tmp_path / "mask.bed", tmp_path / "t.nwk", tmp_path / "u.nwk"
    names = write(fa, seqs)
    bed.write_text("chr\t50\t400\nchr\t%d\t%d\n" % (L - 100, L))
    run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(out), "--mask", str(bed), "--max-n-share", str(F), "--max-sample-n-share", str(G)])
    reduced = np.ascontiguousarray(seqs[kept_samples][:, kept_sites])
    left = [nm for nm, k in zip(names, kept_samples) if k]
    write(tmp_path / "reduced.fa", reduced, names=left)
    run_cli(["--msa", str(tmp_path / "reduced.fa"), "--tree", "nj", "-o", str(out2)])
    assert out.read_text() == out2.read_text()
    check_tree(out.read_text(), left, expected_edges(oracle, reduced))
    # per-site as well: the compared-site counts are the reduced alignment's
    run_cli(["--msa", str(fa), "--tree", "nj", "--tree-distance", "per-site", "-o", str(out), "--mask", str(bed), "--max-n-share", str(F),
             "--max-sample-n-share", str(G)])
    check_tree(out.read_text(), left, expected_edges(oracle, reduced, per_site=True))


def test_a_name_with_a_comma_and_a_quote(hiplib, oracle, base, tmp_path):
    fa, out, ed = tmp_path / "a.fa", tmp_path / "t.nwk", tmp_path / "e.csv"
    seqs = base[:9]
    names = write(fa, seqs, names=["s0", "o'brien,x", "a(b)", "semi;colon", "co:lon", "[x]", "plain", "two''q", "s8"])
    run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(out), "--tree-edges", str(ed)])
    text = out.read_text()
    assert "'o''brien,x':" in text and "'two''''q':" in text and "plain:" in text
    edges = expected_edges(oracle, seqs)
    check_tree(text, names, edges)
    check_edge_rows(ed.read_text().split("\n")[1:-1], names, edges, "a")


@pytest.mark.parametrize("n", [1, 2, 3])
def test_fewer_than_four_samples(hiplib, oracle, base, tmp_path, n):
    fa, out, ed = tmp_path / "a.fa", tmp_path / "t.nwk", tmp_path / "e.csv"
    seqs = base[[3, 30, 50][:n]]
    names = write(fa, seqs, names=["A", "B", "C"][:n])
    run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(out), "--tree-edges", str(ed)])
    D, _ = oracle_matrices(oracle, seqs)
    rows = ed.read_text().split("\n")[1:-1]
    if n == 1:
        assert out.read_text() == "A;\n" and rows == []
    elif n == 2:
        assert D[0, 1] > 0
        half = repr(float(D[0, 1]) / 2).rstrip("0").rstrip(".")
        assert out.read_text() == "(A:%s,B:%s);\n" % (half, half) and rows == ["A,B,%d,a" % D[0, 1]]
    else:
        edges = expected_edges(oracle, seqs)
        check_tree(out.read_text(), names, edges)
        check_edge_rows(rows, names, edges, "a")
        assert out.read_text().startswith("(A:") and out.read_text().count("(") == 1
