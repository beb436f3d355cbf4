"""`tracs distance --tree nj --tree-filter --tree-edges .. --tree-changes .. --tree-filtered ..` end to end (tracs_distance_tree_filter;
DESIGN.md 3.21) on the pinned boundary: alignments of three samples [all A, one case of tests/golden/filter_hp_golden.json, all A].  The
case's changes lie on its sample's terminal edge (with one C among A's the root state is A), so that edge's filtered count is the
fixture's expected count, at 50 digits."""
import json
import os

import numpy as np
import pytest

import hp_filter as H
from test_gpu_tree_changes_cli import run_cli

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PICK = {9000: (90, 600, 1500), 120000: (12, 300, 1200), 600000: (45, 118), 1000000: (196, 4200)}      # a handful of cases per L


@pytest.fixture(scope="module")
def run(tmp_path_factory, hiplib):
    """one run over all the alignments with the filter (the second file on is appended to the first's files), one without"""
    import contextlib
    import io
    d = tmp_path_factory.mktemp("tree_filter")
    with open(os.path.join(HERE, "golden", "filter_hp_golden.json")) as fh:
        cases = [c for c in json.load(fh)["cases"] if c["d"] in PICK[c["L"]]]
    assert len(cases) == 10
    msas = []
    for c in cases:
        L, dd = c["L"], c["d"]
        pos = np.asarray(H.boundary_positions(L, dd, c["row"]), np.int64)
        seq = np.full(L, ord("A"), np.uint8)
        seq[pos] = ord("C")
        fa = d / ("L%dd%d_combined.fasta" % (L, dd))
        fa.write_bytes(b">s0\n" + b"A" * L + b"\n>s1\n" + seq.tobytes() + b"\n>s2\n" + b"A" * L + b"\n")
        msas.append(str(fa))
    f = {k: d / k for k in ("t.nwk", "e.csv", "c.csv", "s.csv", "f.nwk", "plain.nwk", "plain_e.csv", "plain_c.csv", "plain_s.csv")}
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        run_cli(["--msa"] + msas + ["--tree", "nj", "-o", str(f["t.nwk"]), "--tree-filter", "--tree-edges", str(f["e.csv"]), "--tree-changes",
                                    str(f["c.csv"]), "--tree-sites", str(f["s.csv"]), "--tree-filtered", str(f["f.nwk"])])
    run_cli(["--msa"] + msas + ["--tree", "nj", "-o", str(f["plain.nwk"]), "--tree-edges", str(f["plain_e.csv"]), "--tree-changes",
                                str(f["plain_c.csv"]), "--tree-sites", str(f["plain_s.csv"])])
    return {"cases": cases, "msas": msas, "files": f, "stderr": err.getvalue(), "refs": ["L%dd%d" % (c["L"], c["d"]) for c in cases]}


def test_filtered_is_the_pinned_count(run):
    f = run["files"]
    lines = f["e.csv"].read_text().split("\n")
    assert lines[0] == "parent,child,length,changes,filtered,MSA file" and lines[-1] == "" and len(lines) == 2 + 3 * len(run["cases"])
    rows = [r.split(",") for r in lines[1:-1]]
    for k, (c, ref) in enumerate(zip(run["cases"], run["refs"])):
        mine = rows[3 * k:3 * k + 3]
        assert [r[:2] + r[3:] for r in mine] == [["#1", "s0", "0", "0", ref], ["#1", "s1", str(c["d"]), str(c["expected"]), ref],
                                                 ["#1", "s2", "0", "0", ref]], ref
    assert any(0 < c["expected"] < c["d"] for c in run["cases"])


def test_dropped_rows_number_it_and_the_newick_carries_it(run):
    f = run["files"]
    lines = f["c.csv"].read_text().split("\n")
    assert lines[0] == "parent,child,contig,position,alleleParent,alleleChild,dropped,MSA file" and lines[-1] == ""
    rows = [r.split(",") for r in lines[1:-1]]
    trees = f["f.nwk"].read_text().split("\n")
    assert trees[-1] == "" and len(trees) == len(run["cases"]) + 1
    at = 0
    for c, ref, tree in zip(run["cases"], run["refs"], trees):
        mine = rows[at:at + c["d"]]
        at += c["d"]
        pos = H.boundary_positions(c["L"], c["d"], c["row"])
        assert all(r[:3] + r[4:6] + r[7:] == ["#1", "s1", "alignment", "A", "C", ref] for r in mine), ref
        assert [int(r[3]) for r in mine] == list(pos), ref
        assert sum(r[6] == "0" for r in mine) == c["expected"] and all(r[6] in "01" for r in mine), ref
        assert tree == "(s0:0,s1:%d,s2:0);" % c["expected"], ref
        kept = c["expected"]
        assert ("tracs distance: %s: tree filter: %d changes, %d kept, %d dropped, %d branches with a drop\n"
                % (ref, c["d"], kept, c["d"] - kept, int(kept < c["d"]))) in run["stderr"]
    assert at == len(rows)


def test_without_the_flag_the_files_are_what_they_were(run):
    """-o and --tree-sites are byte for byte the filter run's; the edge and change files are the filter run's without the new column,
    under the headers they always had"""
    f = run["files"]
    assert f["plain.nwk"].read_bytes() == f["t.nwk"].read_bytes() and f["plain_s.csv"].read_bytes() == f["s.csv"].read_bytes()
    plain = f["plain_e.csv"].read_text().split("\n")
    assert plain[0] == "parent,child,length,changes,MSA file"
    assert plain[1:] == [",".join(r.split(",")[:4] + r.split(",")[5:]) for r in f["e.csv"].read_text().split("\n")[1:]]
    plain = f["plain_c.csv"].read_text().split("\n")
    assert plain[0] == "parent,child,contig,position,alleleParent,alleleChild,MSA file"
    assert plain[1:] == [",".join(r.split(",")[:6] + r.split(",")[7:]) for r in f["c.csv"].read_text().split("\n")[1:]]


def test_max_entries_is_refused_before_any_file(run, tmp_path):
    """the edge lists count toward --max-entries also without --tree-changes; a file of an earlier run is left as it is"""
    out, ed, fl = (tmp_path / x for x in ("t.nwk", "e.csv", "f.nwk"))
    ed.write_text("earlier\n")
    msa, c = run["msas"][1], run["cases"][1]
    with pytest.raises(SystemExit) as e:
        run_cli(["--msa", msa, "--tree", "nj", "-o", str(out), "--tree-filter", "--tree-edges", str(ed), "--tree-filtered", str(fl),
                 "--max-entries", str(c["d"] - 1)])
    assert "%d changes in all, more than --max-entries %d; nothing was written" % (c["d"], c["d"] - 1) in str(e.value.code)
    assert not out.exists() and not fl.exists() and ed.read_text() == "earlier\n"
    run_cli(["--msa", msa, "--tree", "nj", "-o", str(out), "--tree-filter", "--tree-filtered", str(fl), "--max-entries", str(c["d"])])
    assert fl.read_text() == "(s0:0,s1:%d,s2:0);\n" % c["expected"] and ed.read_text() == "earlier\n"


def test_batches_slabs_and_one_chunk_write_the_same(run, tmp_path, monkeypatch):
    monkeypatch.setenv("TRACS_FITCH_BATCH", "7")
    monkeypatch.setenv("TRACS_FITCH_SLAB_GROUPS", "5")
    monkeypatch.setenv("TRACS_FITCH_MATRIX_CHUNKS", "1")
    out, ed, ch, fl = (tmp_path / x for x in ("t.nwk", "e.csv", "c.csv", "f.nwk"))
    run_cli(["--msa"] + run["msas"][:3] + ["--tree", "nj", "-o", str(out), "--tree-filter", "--tree-edges", str(ed), "--tree-changes", str(ch),
                                           "--tree-filtered", str(fl), "-t", "3"])
    n_rows = sum(c["d"] for c in run["cases"][:3])
    assert ed.read_text().split("\n")[:10] == run["files"]["e.csv"].read_text().split("\n")[:10]
    assert ch.read_text().split("\n")[:n_rows + 1] == run["files"]["c.csv"].read_text().split("\n")[:n_rows + 1]
    assert fl.read_text().split("\n")[:3] == run["files"]["f.nwk"].read_text().split("\n")[:3]
