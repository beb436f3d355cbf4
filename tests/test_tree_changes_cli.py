"""`tracs distance --tree nj --tree-changes FILE --tree-sites FILE [--max-entries N]` on the host: parser defaults, every refusal before
a GPU path is entered, the route, and tracs_tree_write_changes of the cross-compiled library (it touches no device)."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

import nj_ref


def _parser():
    from tracs_amd.distance import distance_parser
    return distance_parser(argparse.ArgumentParser())


def test_defaults_off():
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj"])
    assert a.tree_changes is None and a.tree_sites is None and a.max_entries is None
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj", "--tree-changes", "c.csv", "--tree-sites", "s.csv",
                              "--max-entries", "12"])
    assert (a.tree_changes, a.tree_sites, a.max_entries) == ("c.csv", "s.csv", 12)
    for bad in ("0", "-3", "many"):
        with pytest.raises(SystemExit):
            _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj", "--tree-changes", "c.csv", "--max-entries", bad])


def test_help_says_what_is_unique(capsys):
    with pytest.raises(SystemExit):
        _parser().parse_args(["-h"])
    text = " ".join(capsys.readouterr().out.split())
    for words in ("--tree-changes FILE", "--tree-sites FILE", "--max-entries N", "parsimony length on this tree and is unique",
                  "one most-parsimonious reconstruction among possibly several", "An N sample never carries a change", "homoplasy",
                  "default=100000000"):
        assert words in text, words


def _no_gpu(monkeypatch):
    import tracs_amd.distance as di
    from tracs_amd import _lib, multigpu

    def no_gpu(*a, **k):
        raise AssertionError("a GPU path was entered")
    monkeypatch.setattr(multigpu, "spawn", no_gpu)
    monkeypatch.setattr(multigpu, "init", no_gpu)
    for name in ("nearest_arrays", "pairsnp_arrays", "_rows_on_device", "_forest_on_device", "_histogram_on_device", "_ancestors_on_device",
                 "_tree_on_device"):
        monkeypatch.setattr(di, name, no_gpu)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(_lib, "load", no_gpu)


REFUSALS = [
    (["--tree-changes", "c.csv"], ["--tree-changes", "needs --tree"]),
    (["--tree-sites", "s.csv"], ["--tree-sites", "needs --tree"]),
    (["--max-entries", "5"], ["--max-entries", "needs --tree-changes"]),
    (["--tree", "nj", "--max-entries", "5"], ["--max-entries", "needs --tree-changes"]),
    (["--tree", "nj", "--tree-sites", "s.csv", "--max-entries", "5"], ["--max-entries", "needs --tree-changes"]),
    (["--tree", "nj", "--tree-changes", "c.csv", "--bootstrap", "10"], ["--tree-changes", "--bootstrap", "parent and child"]),
    (["--tree", "nj", "--tree-sites", "s.csv", "--bootstrap", "10"], ["--tree-sites", "--bootstrap", "parent and child"]),
    (["--tree", "nj", "--tree-changes", "c.csv", "--gpus", "2"], ["--tree", "--gpus"]),
    (["--tree", "nj", "--tree-changes", "c.csv", "--filter"], ["--tree", "--filter"]),
]


@pytest.mark.parametrize("extra,words", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_refusals_before_any_gpu_path(tmp_path, monkeypatch, extra, words):
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
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "c.csv") and not os.path.exists(tmp_path / "s.csv")


@pytest.mark.parametrize("own", ["--tree-changes", "--tree-sites"])
def test_the_new_files_must_not_name_another_file_of_the_run(tmp_path, monkeypatch, own):
    _no_gpu(monkeypatch)
    out, edges, other = tmp_path / "o.nwk", tmp_path / "e.csv", tmp_path / "other.csv"
    rest = "--tree-sites" if own == "--tree-changes" else "--tree-changes"
    for clash in (str(out), str(tmp_path / "x.fa"), str(edges), str(other)):
        a = _parser().parse_args(["--msa", str(tmp_path / "x.fa"), "-o", str(out), "--tree", "nj", "--tree-edges", str(edges), own, clash,
                                  rest, str(other)])
        with pytest.raises(SystemExit) as e:
            a.func(a)
        assert "--tree-" in str(e.value.code) and not os.path.exists(out) and not os.path.exists(edges) and not os.path.exists(other)


def test_the_route_creates_no_file_itself(tmp_path, monkeypatch):
    """with --tree-changes the library creates the run's files once the count has passed --max-entries: distance() leaves a stale -o
    and edge file alone and hands the contigs to _tree_on_device; both --tree-distance kinds are taken"""
    import tracs_amd.distance as di
    seen = []
    monkeypatch.setattr(di, "_tree_on_device", lambda msas, args, dates, ref, stage, **kw: seen.append((msas, args.tree_changes, args.tree_distance,
                                                                                                         sorted(kw))))
    fa = tmp_path / "ref1_combined.fasta"
    fa.write_text(">a\nACGT\n>b\nACGA\n")
    out, edges, ch = tmp_path / "o.nwk", tmp_path / "e.csv", tmp_path / "c.csv"
    out.write_text("stale\n")
    for kind in ("snp", "per-site"):
        a = _parser().parse_args(["--msa", str(fa), "-o", str(out), "--tree", "nj", "--tree-edges", str(edges), "--tree-changes", str(ch),
                                  "--tree-distance", kind, "--loglevel", "ERROR"])
        a.func(a)
    assert out.read_text() == "stale\n" and not edges.exists() and not ch.exists()
    assert seen == [([str(fa)], str(ch), "snp", ["tree_contigs"]), ([str(fa)], str(ch), "per-site", ["tree_contigs"])]
    assert di.TREE_EDGES_CHANGES_HEADER == "parent,child,length,changes,MSA file\n"
    assert di.TREE_CHANGES_HEADER == "parent,child,contig,position,alleleParent,alleleChild,MSA file\n"
    assert di.TREE_SITES_HEADER == "contig,position,changes,minimum,MSA file\n"


# ---- the library's host side ------------------------------------------------------------------------------------------------------

def test_library_has_the_fitch_symbols(hiplib):
    from tracs_amd import _lib
    for name in ("tracs_fitch_count", "tracs_fitch_fill", "tracs_tree_write_changes", "tracs_distance_tree_changes"):
        assert hasattr(hiplib, name) and name in _lib.SYMBOLS, name
    assert hiplib.tracs_abi_version() == 1
    assert hiplib.tracs_distance_tree_changes(None, 0, b"x", b"r", None, None, None, None, None, 0, 1, 1, 1, None, None, None, None) == -1
    assert b"tracs_distance_tree_changes" in hiplib.tracs_last_error()
    blob = open(_lib.LIB_PATH, "rb").read()
    for kernel in (b"fitch_leaves_kernel", b"fitch_walk_kernel"):
        assert kernel in blob, kernel


def _write(hiplib, tmp_path, names, parent, child, length, changes, ref="r", edges=True):
    out, ed, plain = tmp_path / "t.nwk", tmp_path / "t.csv", tmp_path / "plain.nwk"
    for p in (out, ed, plain):
        if p.exists():
            p.unlink()
    pa, ch, ln = np.ascontiguousarray(parent, np.uint32), np.ascontiguousarray(child, np.uint32), np.ascontiguousarray(length, np.float64)
    cg = np.ascontiguousarray(changes, np.uint32)
    cn = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    rc = hiplib.tracs_tree_write_changes(cn, len(names), pa.ctypes.data, ch.ctypes.data, ln.ctypes.data, len(pa), cg.ctypes.data,
                                         os.fsencode(str(out)), ref.encode(), os.fsencode(str(ed)) if edges else None)
    if rc:
        raise RuntimeError(hiplib.tracs_last_error().decode())
    assert hiplib.tracs_tree_write(cn, len(names), pa.ctypes.data, ch.ctypes.data, ln.ctypes.data, len(pa), os.fsencode(str(plain)), b"r", None) == 0
    newick = out.read_bytes() if out.exists() else b""
    assert newick == (plain.read_bytes() if plain.exists() else b"")          # tracs_tree_write's line, byte for byte
    return newick.decode(), (ed.read_text() if ed.exists() else "")


def test_newick_and_edge_rows_with_changes(hiplib, tmp_path):
    D = np.array([[0, 5, 9, 9, 8], [5, 0, 10, 10, 9], [9, 10, 0, 8, 7], [9, 10, 8, 0, 3], [8, 9, 7, 3, 0]], np.float64)
    names = ["a", "b", "c", "d", "e"]
    parent, child, length = nj_ref.nj(D)
    text, rows = _write(hiplib, tmp_path, names, parent, child, length, [2, 3, 4, 0, 1, 4000000000, 7], ref="ref1")
    assert text == "(d:2,e:1,(c:4,(a:2,b:3):3):2);\n"
    assert rows == "#1,a,2,2,ref1\n#1,b,3,3,ref1\n#2,c,4,4,ref1\n#2,#1,3,0,ref1\n#3,d,2,1,ref1\n#3,e,1,4000000000,ref1\n#3,#2,2,7,ref1\n"
    text, rows = _write(hiplib, tmp_path, names, parent, child, length, [0] * 7, edges=False)
    assert text == "(d:2,e:1,(c:4,(a:2,b:3):3):2);\n" and rows == ""


def test_small_n_with_changes(hiplib, tmp_path):
    e = np.zeros(0)
    assert _write(hiplib, tmp_path, ["only"], e, e, e, e) == ("only;\n", "")
    assert _write(hiplib, tmp_path, ["A", "B"], [0], [1], [7.0], [5]) == ("(A:3.5,B:3.5);\n", "A,B,7,5,r\n")
    assert _write(hiplib, tmp_path, ["A", "B", "C"], [3, 3, 3], [0, 1, 2], [1.0, 2.0, 4.0], [0, 1, 2]) == \
        ("(A:1,B:2,C:4);\n", "#1,A,1,0,r\n#1,B,2,1,r\n#1,C,4,2,r\n")
    with pytest.raises(RuntimeError, match="2n - 3 edges"):
        _write(hiplib, tmp_path, ["A", "B", "C"], [3, 3], [0, 1], [1.0, 2.0], [0, 0])
