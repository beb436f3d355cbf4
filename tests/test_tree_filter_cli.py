"""`tracs distance --tree nj --tree-filter [--tree-filtered FILE]` on the host: parser defaults, the help text, every
refusal before a GPU path is entered, the route, and tracs_tree_write_filtered of the cross-compiled library (it touches no device)."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

from test_tree_changes_cli import REFUSALS as OLD_REFUSALS
from test_tree_changes_cli import _no_gpu, _parser


def test_defaults_off():
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj"])
    assert a.tree_filter is False and a.tree_filtered is None
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj", "--tree-filter", "--tree-filtered", "f.nwk", "--max-entries", "9"])
    assert (a.tree_filter, a.tree_filtered, a.max_entries) == (True, "f.nwk", 9)


def test_help_says_what_the_filter_does_not_do(capsys):
    with pytest.raises(SystemExit):
        _parser().parse_args(["-h"])
    text = " ".join(capsys.readouterr().out.split())
    for words in ("--tree-filter", "--tree-filtered FILE", "UNFILTERED distances", "not iterated into the topology",
                  "one most-parsimonious reconstruction among possibly several", "filtered column", "dropped column",
                  "With --tree-changes or --tree-filter"):
        assert words in text, words


REFUSALS = [
    (["--tree-filter"], ["--tree-filter", "needs --tree"]),
    (["--tree-filter", "--tree-edges", "e.csv"], ["--tree-edges", "needs --tree"]),
    (["--tree-filtered", "f.nwk"], ["--tree-filtered", "needs --tree-filter"]),
    (["--tree", "nj", "--tree-filter"], ["--tree-filter", "needs --tree-edges, --tree-changes or --tree-filtered"]),
    (["--tree", "nj", "--tree-filter", "--tree-sites", "s.csv"], ["--tree-filter", "needs --tree-edges, --tree-changes or --tree-filtered"]),
    (["--tree", "nj", "--tree-filtered", "f.nwk"], ["--tree-filtered", "needs --tree-filter"]),
    (["--tree", "nj", "--tree-edges", "e.csv", "--tree-filtered", "f.nwk"], ["--tree-filtered", "needs --tree-filter"]),
    (["--tree", "nj", "--tree-filter", "--tree-edges", "e.csv", "--bootstrap", "10"], ["--tree-filter", "--bootstrap", "parent and child"]),
    (["--tree", "nj", "--tree-filter", "--tree-filtered", "f.nwk", "--bootstrap", "10"], ["--tree-filter", "--bootstrap", "parent and child"]),
    (["--tree", "nj", "--tree-filter", "--tree-edges", "e.csv", "--filter"], ["--tree", "--filter"]),
    (["--tree", "nj", "--tree-filter", "--tree-edges", "e.csv", "--gpus", "2"], ["--tree", "--gpus"]),
    (["--tree", "nj", "--tree-filter", "--tree-edges", "e.csv", "--meta", "m.csv"], ["--tree", "--meta"]),
]


@pytest.mark.parametrize("extra,words", REFUSALS + OLD_REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS + OLD_REFUSALS])
def test_refusals_before_any_gpu_path(tmp_path, monkeypatch, extra, words):
    """the new combinations, and the combinations of --tree-changes / --tree-sites / --max-entries with their messages as they were"""
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
    assert not any(os.path.exists(tmp_path / x) for x in ("o.nwk", "c.csv", "s.csv", "e.csv", "f.nwk"))


def test_old_messages_verbatim(tmp_path, monkeypatch):
    _no_gpu(monkeypatch)
    for extra, msg in (
            (["--tree", "nj", "--max-entries", "5"],
             "tracs distance: --max-entries needs --tree-changes (it bounds the rows of that file; --tree-sites has at most one row per site)"),
            (["--max-entries", "5"], "tracs distance: --max-entries needs --tree-changes, which needs --tree (it bounds the rows of that file)"),
            (["--tree", "nj", "--filter"], "tracs distance: --tree is built from the unfiltered SNP distances and takes no --filter")):
        a = _parser().parse_args(["--msa", "x.fa", "-o", str(tmp_path / "o.nwk")] + extra)
        with pytest.raises(SystemExit) as e:
            a.func(a)
        assert str(e.value.code) == msg


def test_max_entries_is_accepted_with_the_filter_alone(tmp_path, monkeypatch):
    """--max-entries bounds the edge lists: accepted with --tree-filter even without --tree-changes; and the route gets the contigs and
    creates no file itself"""
    import tracs_amd.distance as di
    seen = []
    monkeypatch.setattr(di, "_tree_on_device", lambda msas, args, dates, ref, stage, **kw: seen.append((args.tree_filter, args.tree_filtered,
                                                                                                         args.max_entries, sorted(kw))))
    fa = tmp_path / "ref1_combined.fasta"
    fa.write_text(">a\nACGT\n>b\nACGA\n")
    out, ed, fl = tmp_path / "o.nwk", tmp_path / "e.csv", tmp_path / "f.nwk"
    out.write_text("stale\n")
    a = _parser().parse_args(["--msa", str(fa), "-o", str(out), "--tree", "nj", "--tree-filter", "--tree-edges", str(ed), "--tree-filtered", str(fl),
                              "--max-entries", "5", "--loglevel", "ERROR"])
    a.func(a)
    assert seen == [(True, str(fl), 5, ["tree_contigs"])]
    assert out.read_text() == "stale\n" and not ed.exists() and not fl.exists()
    assert di.TREE_EDGES_FILTER_HEADER == "parent,child,length,changes,filtered,MSA file\n"
    assert di.TREE_CHANGES_FILTER_HEADER == "parent,child,contig,position,alleleParent,alleleChild,dropped,MSA file\n"


@pytest.mark.parametrize("clash", ["-o", "--msa", "--tree-edges", "--tree-changes", "--tree-sites"])
def test_tree_filtered_must_not_name_another_file_of_the_run(tmp_path, monkeypatch, clash):
    _no_gpu(monkeypatch)
    paths = {"-o": tmp_path / "o.nwk", "--msa": tmp_path / "x.fa", "--tree-edges": tmp_path / "e.csv", "--tree-changes": tmp_path / "c.csv",
             "--tree-sites": tmp_path / "s.csv"}
    a = _parser().parse_args(["--msa", str(paths["--msa"]), "-o", str(paths["-o"]), "--tree", "nj", "--tree-edges", str(paths["--tree-edges"]),
                              "--tree-changes", str(paths["--tree-changes"]), "--tree-sites", str(paths["--tree-sites"]), "--tree-filter",
                              "--tree-filtered", str(paths[clash])])
    with pytest.raises(SystemExit) as e:
        a.func(a)
    assert "--tree-filtered" in str(e.value.code) and not any(p.exists() for p in paths.values())


def test_handle_refuses_before_the_library(monkeypatch):
    from tracs_amd.handle import DistanceHandle
    h = DistanceHandle.__new__(DistanceHandle)
    h.h = None
    with pytest.raises(ValueError, match="filtered_path needs tree_filter"):
        h.tree("o.nwk", "r", filtered_path="f.nwk")
    with pytest.raises(ValueError, match="tree_filter needs"):
        h.tree("o.nwk", "r", tree_filter=True)
    with pytest.raises(ValueError, match="no bootstrap"):
        h.tree("o.nwk", "r", tree_filter=True, edges_path="e.csv", bootstrap=3)


def test_edge_rows_with_the_filtered_column(hiplib, tmp_path):
    names = ["A", "B", "C"]
    cn = (C.c_char_p * 3)(*[x.encode() for x in names])
    pa, ch = np.array([3, 3, 3], np.uint32), np.array([0, 1, 2], np.uint32)
    ln, cg, kp = np.array([1.0, 2.0, 4.0]), np.array([0, 7, 2], np.uint32), np.array([0, 5, 2], np.uint32)
    out, ed, plain = tmp_path / "t.nwk", tmp_path / "t.csv", tmp_path / "plain.nwk"
    assert hiplib.tracs_tree_write_filtered(cn, 3, pa.ctypes.data, ch.ctypes.data, ln.ctypes.data, 3, cg.ctypes.data, kp.ctypes.data,
                                            os.fsencode(str(out)), b"r", os.fsencode(str(ed))) == 0
    assert hiplib.tracs_tree_write(cn, 3, pa.ctypes.data, ch.ctypes.data, ln.ctypes.data, 3, os.fsencode(str(plain)), b"r", None) == 0
    assert out.read_bytes() == plain.read_bytes() == b"(A:1,B:2,C:4);\n"
    assert ed.read_text() == "#1,A,1,0,0,r\n#1,B,2,7,5,r\n#1,C,4,2,2,r\n"
    assert hiplib.tracs_tree_write_filtered(cn, 3, pa.ctypes.data, ch.ctypes.data, ln.ctypes.data, 3, cg.ctypes.data, None,
                                            os.fsencode(str(out)), b"r", None) == -1
