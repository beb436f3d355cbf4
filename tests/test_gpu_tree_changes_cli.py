"""`tracs distance --tree nj --tree-edges .. --tree-changes .. --tree-sites ..` end to end (tracs_distance_tree_changes; DESIGN.md
3.20): the tree is the run's without the new flags, and the edges' counts, the change rows and the site rows equal tests/fitch_ref.py
on the edges parsed back, in the coordinates of the files read."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

import fitch_ref as fr

pytestmark = pytest.mark.gpu

N, CONTIGS = 12, [("chr1", 400), ("chr2", 300)]
MASKED = [("chr1", 10, 14), ("chr1", 399, 400), ("chr2", 0, 2), ("chr2", 120, 121)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_cli(argv):
    from tracs_amd.distance import distance_parser
    a = distance_parser(argparse.ArgumentParser()).parse_args(argv + ["--loglevel", "ERROR"])
    a.func(a)


def _masks():
    """12 samples x 700 columns around four lineages: ACGT, partial codes and N"""
    rng = np.random.default_rng(2024)
    L = sum(c[1] for c in CONTIGS)
    base = rng.integers(0, 4, L)
    lineage = np.where(rng.random((4, L)) < 0.08, rng.integers(0, 4, (4, L)), base)
    seqs = lineage[np.arange(N) % 4]
    seqs = np.where(rng.random((N, L)) < 0.03, rng.integers(0, 4, (N, L)), seqs)
    masks = (1 << seqs).astype(np.int64)
    masks = np.where(rng.random((N, L)) < 0.04, rng.integers(1, 16, (N, L)), masks)       # partial codes
    return np.where(rng.random((N, L)) < 0.06, 15, masks)


@pytest.fixture(scope="module")
def run(tmp_path_factory, hiplib):
    """the files, one run with the new flags through `python -m tracs_amd` and one without them"""
    d = tmp_path_factory.mktemp("tree_changes")
    masks = _masks()
    names = ["s%02d" % i for i in range(N)]
    fa, ref, bed = d / "ref1_combined.fasta", d / "ref.fa", d / "mask.bed"
    fa.write_text("".join(">%s\n%s\n" % (nm, row) for nm, row in zip(names, fr.masks_to_fasta(masks))))
    ref.write_text("".join(">%s\n%s\n" % (c, "A" * ln) for c, ln in CONTIGS))
    bed.write_text("".join("%s\t%d\t%d\n" % m for m in MASKED))
    keep = np.ones(masks.shape[1], bool)
    start = {"chr1": 0, "chr2": CONTIGS[0][1]}
    for c, b, e in MASKED:
        keep[start[c] + b:start[c] + e] = False
    rules = ["--mask", str(bed), "--mask-reference", str(ref)]
    f = {k: d / k for k in ("t.nwk", "e.csv", "c.csv", "s.csv", "plain.nwk", "plain_e.csv")}
    argv = [sys.executable, "-m", "tracs_amd", "distance", "--msa", str(fa), "--tree", "nj", "-o", str(f["t.nwk"]), "--tree-edges", str(f["e.csv"]),
            "--tree-changes", str(f["c.csv"]), "--tree-sites", str(f["s.csv"]), "--loglevel", "ERROR"] + rules
    p = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(f["plain.nwk"]), "--tree-edges", str(f["plain_e.csv"])] + rules)
    return {"dir": d, "masks": masks, "names": names, "keep": keep, "fa": fa, "rules": rules, "files": f, "stderr": p.stderr}


def _parse_edges(text, names):
    index = {nm: i for i, nm in enumerate(names)}
    node = lambda x: index[x] if x in index else len(names) + int(x[1:]) - 1        # noqa: E731
    rows = [r.split(",") for r in text.splitlines()[1:]]
    return np.array([node(r[0]) for r in rows], np.uint32), np.array([node(r[1]) for r in rows], np.uint32), rows


def _place(col):
    """column of the file read -> (contig, position)"""
    return ("chr1", col) if col < CONTIGS[0][1] else ("chr2", col - CONTIGS[0][1])


def _expected(run):
    f = run["files"]
    parent, child, rows = _parse_edges(f["e.csv"].read_text(), run["names"])
    kept = np.flatnonzero(run["keep"])
    want = fr.fitch(parent, child, run["masks"][:, kept])
    return parent, child, rows, kept, want


def test_the_tree_is_the_run_without_the_new_flags(run):
    f = run["files"]
    assert f["t.nwk"].read_bytes() == f["plain.nwk"].read_bytes() and f["t.nwk"].read_text().count("\n") == 1
    with_changes, plain = f["e.csv"].read_text().splitlines(), f["plain_e.csv"].read_text().splitlines()
    assert with_changes[0] == "parent,child,length,changes,MSA file" and plain[0] == "parent,child,length,MSA file"
    assert len(with_changes) == len(plain) == 2 * N - 3 + 1
    for a, b in zip(with_changes[1:], plain[1:]):
        assert a.split(",")[:3] == b.split(",")[:3] and a.split(",")[4] == b.split(",")[3] == "ref1"


def test_changes_sites_and_edge_counts_equal_the_definition(run):
    f = run["files"]
    parent, child, rows, kept, want = _expected(run)
    assert want["total"] > 50 and (want["site_changes"] > want["site_minimum"]).any()       # (the case has homoplasy to show)
    assert [int(r[3]) for r in rows] == want["edge_changes"].tolist()
    name = lambda v: run["names"][v] if v < N else "#%d" % (v - N + 1)                     # noqa: E731
    letter = {1: "A", 2: "C", 4: "G", 8: "T"}
    lines = f["c.csv"].read_text().split("\n")
    assert lines[0] == "parent,child,contig,position,alleleParent,alleleChild,MSA file" and lines[-1] == ""
    expect = []
    for s, e, info in want["entries"]:
        contig, pos = _place(int(kept[s]))
        expect.append("%s,%s,%s,%d,%s,%s,ref1" % (name(int(parent[e])), name(int(child[e])), contig, pos, letter[info & 15], letter[info >> 4]))
    assert lines[1:-1] == expect
    # no row names a masked column, and rows beyond a masked stretch are shifted back into the file's coordinates
    placed = {(r.split(",")[2], int(r.split(",")[3])) for r in expect}
    assert not any((c, p) in placed for c, b, e in MASKED for p in range(b, e))
    assert any(c == "chr1" and p > 14 for c, p in placed) and any(c == "chr2" and p > 121 for c, p in placed)
    lines = f["s.csv"].read_text().split("\n")
    assert lines[0] == "contig,position,changes,minimum,MSA file" and lines[-1] == ""
    expect = ["%s,%d,%d,%d,ref1" % (_place(int(kept[s])) + (int(want["site_changes"][s]), int(want["site_minimum"][s])))
              for s in np.flatnonzero(want["site_changes"])]
    assert lines[1:-1] == expect
    # the one stderr line: parsimony length, the sum of the minimum over the sites with changes, the consistency index
    changed = want["site_changes"] > 0
    total, low = int(want["total"]), int(want["site_minimum"][changed].sum())
    assert "tracs distance: ref1: parsimony length %d, minimum %d, consistency index %r\n" % (total, low, low / total) in run["stderr"]


def test_max_entries_is_refused_before_any_output_exists(run, tmp_path):
    out, ed, ch, si = (tmp_path / x for x in ("t.nwk", "e.csv", "c.csv", "s.csv"))
    with pytest.raises(SystemExit) as e:
        run_cli(["--msa", str(run["fa"]), "--tree", "nj", "-o", str(out), "--tree-edges", str(ed), "--tree-changes", str(ch), "--tree-sites", str(si),
                 "--max-entries", "1"] + run["rules"])
    total = _expected(run)[4]["total"]
    assert "%d changes in all, more than --max-entries 1; nothing was written" % total in str(e.value.code)
    assert not any(p.exists() for p in (out, ed, ch, si))
    # exactly the total passes
    run_cli(["--msa", str(run["fa"]), "--tree", "nj", "-o", str(out), "--tree-changes", str(ch), "--max-entries", str(total)] + run["rules"])
    assert ch.read_bytes() == run["files"]["c.csv"].read_bytes() and out.read_bytes() == run["files"]["t.nwk"].read_bytes()
    assert not ed.exists() and not si.exists()


def test_batches_of_seven_entries_and_slabs_of_one_group_write_the_same(run, tmp_path, monkeypatch):
    monkeypatch.setenv("TRACS_FITCH_BATCH", "7")
    monkeypatch.setenv("TRACS_FITCH_SLAB_GROUPS", "1")
    out, ed, ch, si = (tmp_path / x for x in ("t.nwk", "e.csv", "c.csv", "s.csv"))
    for p in (out, ch):
        p.write_text("stale\n")                                             # (a file of an earlier run is replaced, not appended to)
    run_cli(["--msa", str(run["fa"]), "--tree", "nj", "-o", str(out), "--tree-edges", str(ed), "--tree-changes", str(ch), "--tree-sites", str(si),
             "-t", "3"] + run["rules"])
    for got, name in ((out, "t.nwk"), (ed, "e.csv"), (ch, "c.csv"), (si, "s.csv")):
        assert got.read_bytes() == run["files"][name].read_bytes(), name


def test_per_site_distances_and_no_rules(run, tmp_path):
    """--tree-distance per-site is taken too, and without a site rule the positions are the alignment's columns"""
    out, ed, ch = (tmp_path / x for x in ("t.nwk", "e.csv", "c.csv"))
    run_cli(["--msa", str(run["fa"]), "--tree", "nj", "--tree-distance", "per-site", "-o", str(out), "--tree-edges", str(ed), "--tree-changes", str(ch)])
    parent, child, rows = _parse_edges(ed.read_text(), run["names"])
    want = fr.fitch(parent, child, run["masks"])
    assert [int(r[3]) for r in rows] == want["edge_changes"].tolist()
    got = [r.split(",") for r in ch.read_text().splitlines()[1:]]
    assert [(r[2], int(r[3])) for r in got] == [("alignment", s) for s, _, _ in want["entries"]]
