"""`tracs distance --tree nj --bootstrap B --bootstrap-support transfer` on the host: parser defaults, every refusal
before a GPU path is entered, the route and the new header, and the host functions of the cross-compiled library
(tracs_tree_transfer_program and tracs_tree_write_transfer touch no device) against tests/transfer_ref.py."""
import argparse
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import bootstrap_ref as br
import nj_ref
import transfer_ref as tr


def _parser():
    from tracs_amd.distance import distance_parser
    return distance_parser(argparse.ArgumentParser())


def test_the_option_is_off_by_default():
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk"])
    assert a.bootstrap_support is None
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj", "--bootstrap", "4"])
    assert a.bootstrap_support is None
    for kind in ("split", "transfer"):
        a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj", "--bootstrap", "4", "--bootstrap-support", kind])
        assert a.bootstrap_support == kind
    with pytest.raises(SystemExit):
        _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj", "--bootstrap", "4", "--bootstrap-support", "felsenstein"])


def test_help_says_what_the_number_is(capsys):
    with pytest.raises(SystemExit):
        _parser().parse_args(["-h"])
    text = " ".join(capsys.readouterr().out.split())
    for words in ("--bootstrap-support {split,transfer}",
                  "smallest number of samples that would have to move",          # what it means
                  "a number in [0, 1], not a count",                              # its range
                  "read the transfer support on branches of positive length only",   # the zero-length caveat
                  "parent,child,length,support,transfer,MSA file"):
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
    (["--bootstrap-support", "transfer"], ["--bootstrap-support", "needs --bootstrap", "needs --tree"]),
    (["--bootstrap-support", "split"], ["--bootstrap-support", "needs --bootstrap", "needs --tree"]),
    (["--tree", "nj", "--bootstrap-support", "transfer"], ["--bootstrap-support", "needs --bootstrap"]),
    (["--tree", "nj", "--bootstrap-support", "split"], ["--bootstrap-support", "needs --bootstrap"]),
    (["--tree", "nj", "--bootstrap", "0", "--bootstrap-support", "transfer"], ["--bootstrap 0", "at least 1"]),
    (["--tree", "nj", "--bootstrap", "4", "--bootstrap-support", "transfer", "--tree-distance", "per-site"], ["--bootstrap", "per-site"]),
    (["--tree", "nj", "--bootstrap", "4", "--bootstrap-support", "transfer", "--gpus", "2"], ["--tree", "--gpus"]),
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
    assert not os.path.exists(out)


def test_transfer_takes_the_tree_route_with_its_own_header(tmp_path, monkeypatch):
    import tracs_amd.distance as di
    seen = []
    monkeypatch.setattr(di, "_tree_on_device", lambda msas, args, dates, ref, stage: seen.append((args.bootstrap, args.bootstrap_support)))
    fa = tmp_path / "ref1_combined.fasta"
    fa.write_text(">a\nACGT\n>b\nACGA\n")
    out, edges = tmp_path / "o.nwk", tmp_path / "e.csv"
    base = ["--msa", str(fa), "-o", str(out), "--tree", "nj", "--tree-edges", str(edges), "--loglevel", "ERROR"]
    a = _parser().parse_args(base + ["--bootstrap", "8", "--bootstrap-support", "transfer"])
    a.func(a)
    assert edges.read_text() == "parent,child,length,support,transfer,MSA file\n" == di.TREE_EDGES_TRANSFER_HEADER
    # without the option, and with its default spelled out, the run writes the header it writes today
    for extra in ([], ["--bootstrap-support", "split"]):
        a = _parser().parse_args(base + ["--bootstrap", "8"] + extra)
        a.func(a)
        assert edges.read_text() == "parent,child,length,support,MSA file\n" == di.TREE_EDGES_SUPPORT_HEADER
    a = _parser().parse_args(base)
    a.func(a)
    assert edges.read_text() == di.TREE_EDGES_HEADER
    assert seen == [(8, "transfer"), (8, None), (8, "split"), (None, None)]


def test_the_handle_chooses_the_entry_point():
    """DistanceHandle.tree() makes one tracs_tree_request of its keywords and calls tracs_distance_tree_run, whatever was asked: support=
    "transfer" is the request's transfer field, the changes and the filter its two flags and four paths"""
    from tracs_amd.handle import DistanceHandle, TreeResult
    calls = []

    class Lib:
        def tracs_distance_tree_run(self, h, req, res):
            q = req._obj
            calls.append({name: getattr(q, name) for name, _ in q._fields_ if not name.startswith("contig_")})
            res._obj.n_joins, res._obj.rows_written, res._obj.n_kept = 5, 13, 2
            return 0
    h = DistanceHandle.__new__(DistanceHandle)
    h.L, h.h = Lib(), None
    assert h.tree("o", "r", bootstrap=4, seed=9) == TreeResult(joins=5, rows=13, changes=0, minimum=0, kept=2, branches=0)
    h.tree("o", "r", bootstrap=4, seed=9, support="transfer", replicate_trees="t")
    h.tree("o", "r", per_site=True, edges_path="e")
    assert [(c["replicates"], c["seed"], c["transfer"]) for c in calls] == [(4, 9, 0), (4, 9, 1), (0, 1, 0)]
    assert [(c["kind"], c["path"], c["ref"], c["edges_path"], c["replicate_trees_path"]) for c in calls] == \
        [(0, b"o", b"r", None, None), (0, b"o", b"r", None, b"t"), (1, b"o", b"r", b"e", None)]
    for c in calls:                                                         # nothing of the changes stage was asked for
        assert (c["changes"], c["filter"], c["changes_path"], c["sites_path"], c["filtered_path"], c["max_entries"]) == (0, 0, None, None, None, 0)
    del calls[:]
    h.tree("o", "r", edges_path="e", changes_path="c", sites_path="s", max_entries=7, n_threads=3, create=False, contigs=[("k", 5)])
    h.tree("o", "r", sites_path="s")
    h.tree("o", "r", edges_path="e", changes_path="c", sites_path="s", tree_filter=True, filtered_path="f")
    h.tree("o", "r", tree_filter=True, filtered_path="f")
    assert [(c["changes"], c["filter"], c["edges_path"], c["changes_path"], c["sites_path"], c["filtered_path"]) for c in calls] == \
        [(1, 0, b"e", b"c", b"s", None), (1, 0, None, None, b"s", None), (1, 1, b"e", b"c", b"s", b"f"), (1, 1, None, None, None, b"f")]
    assert [(c["max_entries"], c["n_threads"], c["create"], c["n_contigs"]) for c in calls] == [(7, 3, 0, 1)] + [(100000000, 0, 1, 0)] * 3
    assert all((c["replicates"], c["transfer"], c["replicate_trees_path"]) == (0, 0, None) for c in calls)
    with pytest.raises(ValueError, match="needs bootstrap"):
        h.tree("o", "r", support="transfer")
    with pytest.raises(ValueError, match="'split' or 'transfer'"):
        h.tree("o", "r", bootstrap=4, support="tbe")
    assert len(calls) == 4                                                  # (a refusal does not reach the library)


# ---- the library's host side ------------------------------------------------------------------------------------------------------

def _program(hiplib, n, edges):
    p, c = (np.ascontiguousarray(x, np.uint32) for x in edges[:2])
    out = np.full(max(2 * n - 3, 1) + 1, 0xDEADBEEF, np.uint32)              # (one guard entry behind the program)
    depth = C.c_size_t(99)
    if hiplib.tracs_tree_transfer_program(n, p.ctypes.data, c.ctypes.data, len(p), out.ctypes.data, C.byref(depth)):
        raise RuntimeError(hiplib.tracs_last_error().decode())
    assert out[-1] == 0xDEADBEEF
    return out[:-1].tolist(), int(depth.value)


def test_library_has_the_transfer_symbols(hiplib):
    from tracs_amd import _lib
    for name in ("tracs_tree_transfer_program", "tracs_transfer_state_bytes", "tracs_transfer_init", "tracs_transfer_add", "tracs_transfer_emit",
                 "tracs_tree_transfer", "tracs_tree_write_transfer", "tracs_distance_tree_bootstrap_transfer"):
        assert hasattr(hiplib, name) and name in _lib.SYMBOLS, name
    assert hiplib.tracs_abi_version() == 1
    assert hiplib.tracs_distance_tree_bootstrap_transfer(None, 0, b"x", b"r", None, 4, 1, None, None, None) == -1
    assert b"tracs_distance_tree_bootstrap_transfer" in hiplib.tracs_last_error()
    assert hiplib.tracs_distance_tree_bootstrap(None, 0, b"x", b"r", None, 4, 1, None, None, None) == -1
    assert hiplib.tracs_last_error().startswith(b"tracs_distance_tree_bootstrap:")
    assert b"transfer_phi_kernel" in open(_lib.LIB_PATH, "rb").read()
    # about n^2 / 8 bytes, and 0 past 2^24 leaves
    assert hiplib.tracs_transfer_state_bytes((1 << 24) + 1) == 0
    got = hiplib.tracs_transfer_state_bytes(10000)
    assert 10000 * 157 * 8 <= got <= 10000 * 157 * 8 + (1 << 20)


def _check_program(n, rep, prog, depth, main):
    assert len(prog) == 2 * n - 3
    leaves = [e for e in prog if not e & tr.INTERNAL]
    assert sorted(leaves) == list(range(n))                                  # every leaf exactly once
    stack, deepest = [], 0
    for e in prog:                                                          # an internal entry carries the size of the two values below it
        if e & tr.INTERNAL:
            b, a = stack.pop(), stack.pop()
            assert a + b == e & ~tr.INTERNAL and a >= b, (a, b, e)         # (largest subtree first)
            stack.append(a + b)
        else:
            stack.append(1)
        deepest = max(deepest, len(stack))
    assert len(stack) == 3 and sum(stack) == n and stack == sorted(stack, reverse=True)
    assert depth == deepest <= int(math.floor(math.log2(n))) + 3, (n, depth)
    assert (prog, depth) == tr.program(n, rep[0], rep[1])                    # the restated builder: the same entries
    want = tr.phi(n, main, rep)
    for e, mask in enumerate(tr.below(n, main[0], main[1])):
        if main[1][e] >= n:
            assert tr.run_program(n, prog, mask)[0] == want[e], (n, e)


@pytest.mark.parametrize("n", [4, 5, 6, 33, 34, 66, 131, 300])
def test_program_on_random_trees(hiplib, n):
    """2n - 3 entries: 63 and 65 (n = 33, 34) lie either side of one 64-entry window, 129 (n = 66) behind the second"""
    rng = np.random.default_rng(100 + n)
    main = br.random_tree_edges(n, rng)
    for rep in [br.random_tree_edges(n, rng), br.random_tree_edges(n, rng), main, nj_ref.nj(nj_ref.random_tree_metric(n, rng)[0])[:2]]:
        prog, depth = _program(hiplib, n, rep)
        _check_program(n, rep, prog, depth, main)


def test_program_of_caterpillars_is_three_deep(hiplib):
    n = 300
    main = br.random_tree_edges(n, np.random.default_rng(7))
    for order in (list(range(n)), list(range(n))[::-1]):
        rep = br.caterpillar_edges(order)
        prog, depth = _program(hiplib, n, rep)
        assert depth == 3
        _check_program(n, rep, prog, depth, main)
    prog, depth = _program(hiplib, 256, tr.balanced_edges(256))
    assert depth == tr.program(256, *tr.balanced_edges(256))[1] <= 11 and depth >= 8      # the deepest shape


def test_program_of_a_20000_leaf_caterpillar_needs_no_recursion(hiplib):
    n = 20000
    for order in (list(range(n)), list(range(n))[::-1]):
        prog, depth = _program(hiplib, n, br.caterpillar_edges(order))
        assert depth == 3 and len(prog) == 2 * n - 3
        assert sorted(e for e in prog if not e & tr.INTERNAL) == list(range(n))
        assert [e & ~tr.INTERNAL for e in prog if e & tr.INTERNAL] == list(range(2, n - 1))


def test_program_refuses_malformed_edges(hiplib):
    main = br.random_tree_edges(6, np.random.default_rng(0))
    assert _program(hiplib, 3, (np.array([3, 3, 3]), np.array([0, 1, 2])))[1] == 0          # n < 4: nothing to do
    with pytest.raises(RuntimeError, match="2n - 3 edges"):
        _program(hiplib, 6, (main[0][:-1], main[1][:-1]))
    bad = (main[0].copy(), main[1].copy())
    bad[1][0] = bad[1][1]
    with pytest.raises(RuntimeError, match="not a tree in creation order"):
        _program(hiplib, 6, bad)
    with pytest.raises(RuntimeError, match="not a tree in creation order"):
        _program(hiplib, 6, (main[0][::-1].copy(), main[1][::-1].copy()))
    # 2n - 3 edges that hang every node once, but a joined node with three children and a top node with two
    lopsided = (np.array([6, 6, 6, 7, 7, 8, 8, 9, 9], np.uint32), np.array([0, 1, 2, 3, 6, 4, 7, 5, 8], np.uint32))
    with pytest.raises(RuntimeError, match="not a tree in creation order"):
        _program(hiplib, 6, lopsided)
    assert hiplib.tracs_tree_transfer_program(6, None, None, 9, None, None) == -1


def _write(hiplib, tmp_path, names, parent, child, length, support, sum_phi, light, replicates, ref="r"):
    out, ed = tmp_path / "t.nwk", tmp_path / "t.csv"
    for p in (out, ed):
        if p.exists():
            p.unlink()
    pa, ch, ln = np.ascontiguousarray(parent, np.uint32), np.ascontiguousarray(child, np.uint32), np.ascontiguousarray(length, np.float64)
    su, sp, li = np.ascontiguousarray(support, np.uint32), np.ascontiguousarray(sum_phi, np.uint64), np.ascontiguousarray(light, np.uint32)
    cn = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    rc = hiplib.tracs_tree_write_transfer(cn, len(names), pa.ctypes.data, ch.ctypes.data, ln.ctypes.data, len(pa), su.ctypes.data, sp.ctypes.data,
                                          li.ctypes.data, replicates, os.fsencode(str(out)), ref.encode(), os.fsencode(str(ed)))
    if rc:
        raise RuntimeError(hiplib.tracs_last_error().decode())
    return out.read_text() if out.exists() else "", (ed.read_text() if ed.exists() else "")


def _plain(hiplib, tmp_path, names, parent, child, length):
    out = tmp_path / "plain.nwk"
    if out.exists():
        out.unlink()
    pa, ch, ln = np.ascontiguousarray(parent, np.uint32), np.ascontiguousarray(child, np.uint32), np.ascontiguousarray(length, np.float64)
    cn = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    assert hiplib.tracs_tree_write(cn, len(names), pa.ctypes.data, ch.ctypes.data, ln.ctypes.data, len(pa), os.fsencode(str(out)), b"r", None) == 0
    return out.read_text()


LABEL = re.compile(r"\)([0-9][0-9.e+-]*):")


def test_newick_with_transfer_support_of_a_small_tree_and_its_edge_rows(hiplib, tmp_path):
    D = np.array([[0, 5, 9, 9, 8], [5, 0, 10, 10, 9], [9, 10, 0, 8, 7], [9, 10, 8, 0, 3], [8, 9, 7, 3, 0]], np.float64)
    names = ["a", "b", "c", "d", "e"]
    parent, child, length = nj_ref.nj(D)                                    # edges 3 and 6 are internal, both with a lighter side of 2
    none = br.NONE
    text, rows = _write(hiplib, tmp_path, names, parent, child, length, [none, none, none, 5, none, none, 8], [9, 9, 9, 1, 9, 9, 0], [7, 7, 7, 2, 7, 7, 2],
                        8, ref="ref1")
    assert text == "(d:2,e:1,(c:4,(a:2,b:3)0.875:3)1:2);\n"
    assert rows == ("#1,a,2,NA,NA,ref1\n#1,b,3,NA,NA,ref1\n#2,c,4,NA,NA,ref1\n#2,#1,3,5,0.875,ref1\n#3,d,2,NA,NA,ref1\n#3,e,1,NA,NA,ref1\n"
                    "#3,#2,2,8,1,ref1\n")
    # the shortest form that reads back: 1 - 1/3 and 0
    text, rows = _write(hiplib, tmp_path, names, parent, child, length, [none, none, none, 0, none, none, 0], [0, 0, 0, 1, 0, 0, 3], [0, 0, 0, 2, 0, 0, 2], 3)
    assert text == "(d:2,e:1,(c:4,(a:2,b:3)%s:3)0:2);\n" % repr(1.0 - float(1) / float(3))
    assert float(rows.splitlines()[3].split(",")[4]) == 1.0 - float(1) / float(3) and rows.splitlines()[6].split(",")[3:5] == ["0", "0"]
    # labels on internal nodes only, and with them stripped the line is tracs_tree_write's
    assert LABEL.sub("):", text) == "(d:2,e:1,(c:4,(a:2,b:3):3):2);\n" == _plain(hiplib, tmp_path, names, parent, child, length)
    nodes = nj_ref.parse_newick(text)
    kids = {p for p, _, _ in nodes}
    assert all((k in kids) == (lab not in names) for k, (_, lab, _) in enumerate(nodes))
    # what cannot be a transfer support is refused
    with pytest.raises(RuntimeError, match="9 out of 8"):
        _write(hiplib, tmp_path, names, parent, child, length, [none, none, none, 9, none, none, 1], [0] * 7, [2] * 7, 8)
    with pytest.raises(RuntimeError, match="lighter side"):
        _write(hiplib, tmp_path, names, parent, child, length, [0] * 7, [0, 0, 0, 9, 0, 0, 0], [2] * 7, 8)      # Phi > B (p - 1)
    with pytest.raises(RuntimeError, match="lighter side"):
        _write(hiplib, tmp_path, names, parent, child, length, [0] * 7, [0] * 7, [1] * 7, 8)                     # p < 2


def test_small_n_and_quoting_with_transfer_support(hiplib, tmp_path):
    e = np.zeros(0)
    assert _write(hiplib, tmp_path, ["only"], e, e, e, e, e, e, 4) == ("only;\n", "")
    assert _write(hiplib, tmp_path, ["A", "B"], [0], [1], [7.0], [br.NONE], [0], [0], 4) == ("(A:3.5,B:3.5);\n", "A,B,7,NA,NA,r\n")
    assert _write(hiplib, tmp_path, ["A", "B", "C"], [3, 3, 3], [0, 1, 2], [1.0, 2.0, 4.0], [br.NONE] * 3, [0] * 3, [0] * 3, 4) == \
        ("(A:1,B:2,C:4);\n", "#1,A,1,NA,NA,r\n#1,B,2,NA,NA,r\n#1,C,4,NA,NA,r\n")
    names = ["plain_1.2-x", "with space", "it's", "a,b", "semi;colon", "(paren)", "[br]", "co:lon", "tab\there"]
    n = len(names)
    parent, child, length = nj_ref.nj(nj_ref.random_tree_metric(n, np.random.default_rng(1))[0])
    main = (parent, child)
    light = np.array([2 if x == tr.NONE else x for x in tr.light(n, main)], np.uint32)
    text, _ = _write(hiplib, tmp_path, names, parent, child, length, np.where(child >= n, 5, br.NONE), np.where(child >= n, 5, 0), light, 5)
    for want in ("plain_1.2-x:", "'with space':", "'it''s':", "'a,b':", "'semi;colon':", "'(paren)':", "'[br]':", "'co:lon':", "'tab\there':"):
        assert want in text, want
    assert "'plain" not in text and len(LABEL.findall(text)) == n - 3
    assert LABEL.sub("):", text) == _plain(hiplib, tmp_path, names, parent, child, length)


# ---- the definition on the fixture ------------------------------------------------------------------------------------------------

def test_the_restatement_on_the_outbreak_fixture():
    seqs = br.outbreak_alignment()
    n = seqs.shape[0]
    main = nj_ref.nj(br.snp_matrix(seqs).astype(np.float64))
    reps = [br.replicate_tree(seqs, 3, b) for b in range(8)]
    split = br.supports(n, main, reps)
    sums, p, x = tr.transfer(n, main, reps)
    assert (int(split[43]), sums[43], p[43], x[43]) == (0, 21, 10, 0.7083333333333333)
    assert int(split[41]) == 1 and x[41] == 0.7727272727272727
    assert int(split[25]) == int(split[33]) == 8 and x[25] == x[33] == 1.0 and sums[25] == sums[33] == 0
    inner = [v for v in x if v == v]
    assert len(inner) == n - 3 and min(inner) == 0.4375 and max(inner) == 1.0
    # phi = 0 exactly where the replicate has the split, and a tree against itself has every split
    for b, rep in enumerate(reps):
        has = br.supports(n, main, [rep])
        assert all((f == 0) == (int(h) == 1) for f, h, c in zip(tr.phi(n, main, rep), has, main[1]) if c >= n), b
    sums, _, x = tr.transfer(n, main, [main, main])
    assert all(s == 0 and v == 1.0 for s, v, c in zip(sums, x, main[1]) if c >= n)
