"""`tracs distance --tree nj [--tree-distance] [--tree-edges]` on the host: parser defaults, every refusal before a GPU path is entered,
the route, and the Newick writer of the cross-compiled library (tracs_nj_edges / tracs_tree_write touch no device)."""
import argparse
import ctypes as C
import os
import struct

import numpy as np
import pytest

import nj_ref


def _parser():
    from tracs_amd.distance import distance_parser
    return distance_parser(argparse.ArgumentParser())


def test_defaults_off():
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk"])
    assert a.tree is None and a.tree_distance is None and a.tree_edges is None
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj", "--tree-distance", "per-site", "--tree-edges", "e.csv"])
    assert (a.tree, a.tree_distance, a.tree_edges) == ("nj", "per-site", "e.csv")
    with pytest.raises(SystemExit):
        _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "upgma"])


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
    (["--tree-distance", "snp"], ["--tree-distance", "needs --tree"]),
    (["--tree-edges", "e.csv"], ["--tree-edges", "needs --tree"]),
    (["--tree", "nj", "--nearest", "3"], ["--tree", "--nearest"]),
    (["--tree", "nj", "--mst", "snp"], ["--tree", "--mst"]),
    (["--tree", "nj", "--ancestors", "snp", "--meta", "m.csv"], ["--tree", "--ancestors"]),
    (["--tree", "nj", "--histogram"], ["--tree", "--histogram"]),
    (["--tree", "nj", "-D", "10"], ["--tree", "-D"]),
    (["--tree", "nj", "-K", "3"], ["--tree", "-K"]),
    (["--tree", "nj", "--filter"], ["--tree", "--filter"]),
    (["--tree", "nj", "--meta", "m.csv"], ["--tree", "--meta"]),
    (["--tree", "nj", "--min-sites", "10"], ["--tree", "--min-sites"]),
    (["--tree", "nj", "--msa-db", "db.fa"], ["--tree", "--msa-db"]),
    (["--tree", "nj", "--gpus", "2"], ["--tree", "--gpus"]),
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
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "e.csv")


def test_tree_edges_must_not_name_another_file_of_the_run(tmp_path, monkeypatch):
    _no_gpu(monkeypatch)
    out = tmp_path / "o.nwk"
    for edges in (str(out), str(tmp_path / "x.fa")):
        a = _parser().parse_args(["--msa", str(tmp_path / "x.fa"), "-o", str(out), "--tree", "nj", "--tree-edges", edges])
        with pytest.raises(SystemExit) as e:
            a.func(a)
        assert "--tree-edges" in str(e.value.code) and not os.path.exists(out)


def test_tree_takes_its_own_route(tmp_path, monkeypatch):
    """--tree writes no header into -o, the edges header into --tree-edges, and hands each --msa file to _tree_on_device"""
    import tracs_amd.distance as di
    seen = []

    def refuse(*a, **k):
        raise AssertionError("--tree must not take a pair route")
    for name in ("nearest_arrays", "pairsnp_arrays", "_rows_on_device", "_forest_on_device", "_histogram_on_device"):
        monkeypatch.setattr(di, name, refuse)
    monkeypatch.setattr(di, "_tree_on_device", lambda msas, args, dates, ref, stage: seen.append((msas, dates, ref)))
    fa, fb = tmp_path / "ref1_combined.fasta", tmp_path / "ref2.fasta.gz"
    for p in (fa, fb):
        p.write_text(">a\nACGT\n>b\nACGA\n")
    out, edges = tmp_path / "o.nwk", tmp_path / "e.csv"
    a = _parser().parse_args(["--msa", str(fa), str(fb), "-o", str(out), "--tree", "nj", "--tree-edges", str(edges), "--loglevel", "ERROR"])
    a.func(a)
    assert out.read_text() == "" and edges.read_text() == "parent,child,length,MSA file\n" == di.TREE_EDGES_HEADER
    assert seen == [([str(fa)], None, "ref1"), ([str(fb)], None, "ref2")]
    assert di.DEVICE_ROUTES["tree"][0] == "_tree_on_device" and len(di.DEVICE_ROUTES) == 4


# ---- the library's host side ------------------------------------------------------------------------------------------------------

def _write(hiplib, tmp_path, names, parent, child, length, ref="r", edges=True):
    from tracs_amd import _lib
    out, ed = tmp_path / "t.nwk", tmp_path / "t.csv"
    for p in (out, ed):
        if p.exists():
            p.unlink()
    pa, ch, ln = np.ascontiguousarray(parent, np.uint32), np.ascontiguousarray(child, np.uint32), np.ascontiguousarray(length, np.float64)
    cn = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    rc = hiplib.tracs_tree_write(cn, len(names), pa.ctypes.data, ch.ctypes.data, ln.ctypes.data, len(pa), os.fsencode(str(out)), ref.encode(),
                                 os.fsencode(str(ed)) if edges else None)
    if rc:
        raise RuntimeError(hiplib.tracs_last_error().decode())
    return out.read_text() if out.exists() else "", (ed.read_text() if ed.exists() else "")


def _edges(hiplib, n, rec, last_ids, last_d):
    from tracs_amd import device as dev            # (tracs_nj_edges is host code: no GPU is asked for)
    return dev.nj_edges(n, rec, last_ids, last_d)


def test_library_has_the_tree_symbols(hiplib):
    from tracs_amd import _lib
    names = ["tracs_nj_state_bytes", "tracs_nj_init", "tracs_nj_load_panel", "tracs_nj_load_f64", "tracs_nj_run", "tracs_nj_emit",
             "tracs_nj_edges", "tracs_tree_write", "tracs_distance_tree"]
    for name in names:
        assert hasattr(hiplib, name) and name in _lib.SYMBOLS, name
    assert hiplib.tracs_nj_state_bytes(0) > 0 and hiplib.tracs_nj_state_bytes(2 ** 24 + 1) == 0
    assert 8 * 10000 ** 2 <= hiplib.tracs_nj_state_bytes(10000) < 8 * 10000 ** 2 + (1 << 20)
    assert hiplib.tracs_nj_init(None, 10, None) == -1 and b"tracs_nj_init" in hiplib.tracs_last_error()
    assert hiplib.tracs_nj_run(None, 10, None) == -1
    assert hiplib.tracs_distance_tree(None, 0, b"x", b"r", None, None, None) == -1
    assert hiplib.tracs_abi_version() == 1
    blob = open(_lib.LIB_PATH, "rb").read()
    for kernel in (b"nj_scan_kernel", b"nj_rows_kernel", b"nj_commit_kernel", b"nj_rowsum_kernel", b"nj_load_kernel"):
        assert kernel in blob, kernel


def test_library_lengths_are_the_definitions(hiplib):
    rng = np.random.default_rng(3)
    for n in (2, 3, 4, 9, 40):
        U = np.triu(rng.integers(0, 1000, (n, n)), 1)
        D = (U + U.T).astype(np.float64) / 7.0
        rec, ids, d = nj_ref.nj_records(D)
        got, want = _edges(hiplib, n, rec, ids, d), nj_ref.nj_edges(n, rec, ids, d)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), n


def test_newick_of_a_small_tree_and_its_edge_rows(hiplib, tmp_path):
    D = np.array([[0, 5, 9, 9, 8], [5, 0, 10, 10, 9], [9, 10, 0, 8, 7], [9, 10, 8, 0, 3], [8, 9, 7, 3, 0]], np.float64)   # the textbook five-taxon example: a:2, b:3, c:4, d:2, e:1 and inner branches 3 and 2
    names = ["a", "b", "c", "d", "e"]
    rec, ids, d = nj_ref.nj_records(D)
    parent, child, length = _edges(hiplib, 5, rec, ids, d)
    text, rows = _write(hiplib, tmp_path, names, parent, child, length, ref="ref1")
    assert text == "(d:2,e:1,(c:4,(a:2,b:3):3):2);\n"
    assert rows == "#1,a,2,ref1\n#1,b,3,ref1\n#2,c,4,ref1\n#2,#1,3,ref1\n#3,d,2,ref1\n#3,e,1,ref1\n#3,#2,2,ref1\n"
    sp = nj_ref.newick_splits(nj_ref.parse_newick(text), names)
    assert sp == nj_ref.splits_of(5, parent, child, length)


def test_small_n(hiplib, tmp_path):
    e = np.zeros(0)
    assert _write(hiplib, tmp_path, ["only"], e, e, e) == ("only;\n", "")
    assert _write(hiplib, tmp_path, ["A", "B"], [0], [1], [7.0]) == ("(A:3.5,B:3.5);\n", "A,B,7,r\n")
    assert _write(hiplib, tmp_path, ["A", "B", "C"], [3, 3, 3], [0, 1, 2], [1.0, 2.0, 4.0]) == ("(A:1,B:2,C:4);\n", "#1,A,1,r\n#1,B,2,r\n#1,C,4,r\n")
    assert _write(hiplib, tmp_path, [], e, e, e, edges=False) == ("", "")
    with pytest.raises(RuntimeError, match="2n - 3 edges"):
        _write(hiplib, tmp_path, ["A", "B", "C"], [3, 3], [0, 1], [1.0, 2.0])
    with pytest.raises(RuntimeError, match="not a tree"):
        _write(hiplib, tmp_path, ["A", "B", "C"], [3, 3, 3], [0, 1, 1], [1.0, 2.0, 4.0])


def test_names_are_quoted_where_newick_needs_it(hiplib, tmp_path):
    names = ["plain_1.2-x", "with space", "it's", "a,b", "semi;colon", "(paren)", "[br]", "co:lon", "tab\there"]
    n = len(names)
    D = nj_ref.random_tree_metric(n, np.random.default_rng(1))[0]
    rec, ids, d = nj_ref.nj_records(D)
    parent, child, length = _edges(hiplib, n, rec, ids, d)
    text, _ = _write(hiplib, tmp_path, names, parent, child, length)
    for want in ("plain_1.2-x:", "'with space':", "'it''s':", "'a,b':", "'semi;colon':", "'(paren)':", "'[br]':", "'co:lon':", "'tab\there':"):
        assert want in text, want
    assert "'plain" not in text
    nodes = nj_ref.parse_newick(text)
    assert nj_ref.newick_splits(nodes, names) == nj_ref.splits_of(n, parent, child, length)      # every name round-trips


def test_lengths_are_the_shortest_text_that_reads_back(hiplib, tmp_path):
    rng = np.random.default_rng(9)
    vals = [0.0, -0.0, 1.0, -2.5, 0.1, 1 / 3, 2 / 3, 1e-5, 1e22, 123456789.0, 5e-324, 1.7976931348623157e308, 0.30000000000000004, 2.0 ** 53,
            7.0 / 65536] + [struct.unpack("<d", struct.pack("<Q", int(b)))[0] for b in rng.integers(1 << 52, 0x7FE << 52, 200, dtype=np.uint64)]
    for k in range(0, len(vals), 3):
        x = (vals[k:k + 3] + [1.0, 1.0])[:3]
        text, rows = _write(hiplib, tmp_path, ["A", "B", "C"], [3, 3, 3], [0, 1, 2], x)
        got = [ln for _, lab, ln in nj_ref.parse_newick(text)[1:]]
        fields = [r.split(",")[2] for r in rows.splitlines()]
        for v, g, f in zip(x, got, fields):
            assert struct.pack("<d", g) == struct.pack("<d", v) and struct.pack("<d", float(f)) == struct.pack("<d", v), (v, f)
            assert len(f) <= len(repr(v)), (v, f)                      # never longer than Python's shortest round-trip repr


def test_a_20000_leaf_caterpillar_needs_no_recursion(hiplib, tmp_path):
    """joins (0, 1), (2, n), (3, n + 1), ...: every join hangs the next leaf beside the node before it, so the tree is n deep"""
    n = 20000
    names = ["s%d" % k for k in range(n)]
    a = np.array([0] + list(range(2, n - 2)), np.uint32)
    b = np.array([1] + list(range(n, 2 * n - 4)), np.uint32)
    dab = np.full(n - 3, 2.0)
    r = np.zeros(n - 3)
    last_ids, last_d = np.array([n - 2, n - 1, 2 * n - 4], np.uint32), np.array([2.0, 2.0, 2.0])
    parent, child, length = _edges(hiplib, n, (a, b, dab, r, r), last_ids, last_d)
    assert len(parent) == 2 * n - 3 and (length == 1.0).all()
    text, rows = _write(hiplib, tmp_path, names, parent, child, length)
    assert text.count("(") == text.count(")") == n - 2 and text.endswith(";\n") and text.count("\n") == 1
    depth = best = 0
    for ch in text:
        depth += ch == "("
        depth -= ch == ")"
        best = max(best, depth)
    assert best == n - 2
    nodes = nj_ref.parse_newick(text)
    assert sorted(lab for _, lab, _ in nodes if lab is not None) == sorted(names)
    assert sum(1 for _, lab, _ in nodes if lab is None) == n - 2 and all(ln == 1.0 for p, _, ln in nodes if p is not None)
    assert rows.count("\n") == 2 * n - 3 and rows.endswith("#%d,#%d,1,r\n" % (n - 2, n - 3))
