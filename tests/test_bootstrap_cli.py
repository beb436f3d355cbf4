"""`tracs distance --tree nj --bootstrap B [--bootstrap-seed S] [--bootstrap-trees FILE]` on the host: parser defaults, every refusal
before a GPU path is entered, the route, and the host functions of the cross-compiled library (tracs_tree_support and
tracs_tree_write_support touch no device) against tests/bootstrap_ref.py."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

import bootstrap_ref as br
import nj_ref


def _parser():
    from tracs_amd.distance import distance_parser
    return distance_parser(argparse.ArgumentParser())


def test_defaults_off():
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk"])
    assert a.bootstrap is None and a.bootstrap_seed is None and a.bootstrap_trees is None
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj"])
    assert a.bootstrap is None and a.bootstrap_seed is None and a.bootstrap_trees is None
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj", "--bootstrap", "100", "--bootstrap-seed", str(2 ** 64 - 1),
                              "--bootstrap-trees", "b.nwk"])
    assert (a.bootstrap, a.bootstrap_seed, a.bootstrap_trees) == (100, 2 ** 64 - 1, "b.nwk")
    with pytest.raises(SystemExit):
        _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj", "--bootstrap", "many"])


def test_help_says_what_the_label_is(capsys):
    with pytest.raises(SystemExit):
        _parser().parse_args(["-h"])
    text = " ".join(capsys.readouterr().out.split())
    for words in ("--bootstrap B", "--bootstrap-seed S", "--bootstrap-trees FILE", "a count out of B", "reproducible bit for bit",
                  "broken by input order in every replicate", "shows support B", "branches of positive length"):
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
    (["--bootstrap", "10"], ["--bootstrap", "needs --tree"]),
    (["--bootstrap-seed", "3"], ["--bootstrap-seed", "needs --tree"]),
    (["--bootstrap-trees", "b.nwk"], ["--bootstrap-trees", "needs --tree"]),
    (["--tree", "nj", "--bootstrap-seed", "3"], ["--bootstrap-seed", "needs --bootstrap"]),
    (["--tree", "nj", "--bootstrap-trees", "b.nwk"], ["--bootstrap-trees", "needs --bootstrap"]),
    (["--tree", "nj", "--bootstrap", "0"], ["--bootstrap 0", "at least 1"]),
    (["--tree", "nj", "--bootstrap", "-5"], ["--bootstrap -5", "at least 1"]),
    (["--tree", "nj", "--bootstrap", "10", "--bootstrap-seed", "-1"], ["--bootstrap-seed", "2^64"]),
    (["--tree", "nj", "--bootstrap", "10", "--bootstrap-seed", str(2 ** 64)], ["--bootstrap-seed", "2^64"]),
    (["--tree", "nj", "--bootstrap", "10", "--tree-distance", "per-site"], ["--bootstrap", "--tree-distance per-site"]),
    (["--tree", "nj", "--bootstrap", "10", "--gpus", "2"], ["--tree", "--gpus"]),
    (["--tree", "nj", "--bootstrap", "10", "-D", "5"], ["--tree", "-D"]),
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
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "b.nwk")


def test_bootstrap_trees_must_not_name_another_file_of_the_run(tmp_path, monkeypatch):
    _no_gpu(monkeypatch)
    out, edges = tmp_path / "o.nwk", tmp_path / "e.csv"
    for trees in (str(out), str(tmp_path / "x.fa"), str(edges)):
        a = _parser().parse_args(["--msa", str(tmp_path / "x.fa"), "-o", str(out), "--tree", "nj", "--tree-edges", str(edges), "--bootstrap", "4",
                                  "--bootstrap-trees", trees])
        with pytest.raises(SystemExit) as e:
            a.func(a)
        assert "--bootstrap-trees" in str(e.value.code) and not os.path.exists(out) and not os.path.exists(edges)


def test_bootstrap_takes_the_tree_route(tmp_path, monkeypatch):
    """--bootstrap writes the edges header with its support column, truncates --bootstrap-trees, and goes to _tree_on_device"""
    import tracs_amd.distance as di
    seen = []
    monkeypatch.setattr(di, "_tree_on_device", lambda msas, args, dates, ref, stage: seen.append((msas, args.bootstrap, args.bootstrap_seed)))
    fa = tmp_path / "ref1_combined.fasta"
    fa.write_text(">a\nACGT\n>b\nACGA\n")
    out, edges, trees = tmp_path / "o.nwk", tmp_path / "e.csv", tmp_path / "b.nwk"
    trees.write_text("stale\n")
    a = _parser().parse_args(["--msa", str(fa), "-o", str(out), "--tree", "nj", "--tree-edges", str(edges), "--bootstrap", "8",
                              "--bootstrap-trees", str(trees), "--loglevel", "ERROR"])
    a.func(a)
    assert out.read_text() == "" and trees.read_text() == ""
    assert edges.read_text() == "parent,child,length,support,MSA file\n" == di.TREE_EDGES_SUPPORT_HEADER
    assert seen == [([str(fa)], 8, None)]
    # without --bootstrap the header is the old one
    a = _parser().parse_args(["--msa", str(fa), "-o", str(out), "--tree", "nj", "--tree-edges", str(edges), "--loglevel", "ERROR"])
    a.func(a)
    assert edges.read_text() == "parent,child,length,MSA file\n"


# ---- the library's host side ------------------------------------------------------------------------------------------------------

def _support(hiplib, n, main, reps, count=None):
    p, c = (np.ascontiguousarray(x, np.uint32) for x in main[:2])
    count = np.zeros(len(p), np.uint32) if count is None else count
    for rep in reps:
        rp, rc = (np.ascontiguousarray(x, np.uint32) for x in rep[:2])
        rc_ = hiplib.tracs_tree_support(n, p.ctypes.data, c.ctypes.data, len(p), rp.ctypes.data, rc.ctypes.data, len(rp), count.ctypes.data)
        if rc_:
            raise RuntimeError(hiplib.tracs_last_error().decode())
    return count


def _want(n, main, reps):
    w = br.supports(n, main, reps)
    w[w == br.NONE] = 0                                                     # (the library leaves the leaf edges' counts alone)
    return w


def test_library_has_the_bootstrap_symbols(hiplib):
    from tracs_amd import _lib
    for name in ("tracs_bootstrap_weights", "tracs_alignment_gather_sites", "tracs_tree_support", "tracs_tree_write_support",
                 "tracs_distance_tree_bootstrap"):
        assert hasattr(hiplib, name) and name in _lib.SYMBOLS, name
    assert hiplib.tracs_abi_version() == 1
    assert hiplib.tracs_distance_tree_bootstrap(None, 0, b"x", b"r", None, 4, 1, None, None, None) == -1
    assert b"tracs_distance_tree_bootstrap" in hiplib.tracs_last_error()
    blob = open(_lib.LIB_PATH, "rb").read()
    for kernel in (b"bootstrap_weights_kernel", b"gather_sites_kernel"):
        assert kernel in blob, kernel


@pytest.mark.parametrize("n", [4, 5, 6, 64, 65, 129])
def test_support_on_random_trees(hiplib, n):
    """the word boundaries of the bitsets: n = 64 fills one word, 65 and 129 start another"""
    rng = np.random.default_rng(n)
    main = br.random_tree_edges(n, rng)
    internal = main[1] >= n
    assert internal.sum() == n - 3
    # the replicate equal to the main tree: every internal edge + 1, nothing else touched
    got = _support(hiplib, n, main, [main])
    assert np.array_equal(got, internal.astype(np.uint32))
    got = _support(hiplib, n, main, [main], count=np.full(len(main[0]), 5, np.uint32))
    assert np.array_equal(got, 5 + internal.astype(np.uint32))
    # random trees, trees that share subtrees with the main one, and a caterpillar in reversed leaf order
    reps = [br.random_tree_edges(n, rng) for _ in range(4)] + [br.caterpillar_edges(list(range(n))[::-1]), br.caterpillar_edges(list(range(n)))]
    D = nj_ref.random_tree_metric(n, rng)[0]
    noise = [np.triu(rng.integers(0, 3, (n, n)), 1).astype(np.float64) for _ in range(2)]
    near = [nj_ref.nj(D + N + N.T)[:2] for N in noise]
    base = nj_ref.nj(D)[:2]
    got = _support(hiplib, n, base, reps + near + [base])
    want = _want(n, base, reps + near + [base])
    assert np.array_equal(got, want), (got, want)
    assert want[base[1] >= n].min() >= 1
    # the caterpillars against each other: the same splits, whichever end they were built from
    a, b = br.caterpillar_edges(list(range(n))), br.caterpillar_edges(list(range(n))[::-1])
    assert np.array_equal(_support(hiplib, n, a, [b]), _want(n, a, [b])) and _want(n, a, [b]).sum() == n - 3
    # the Python entry point
    from tracs_amd import api
    assert np.array_equal(api.tree_support(n, base, reps + near + [base]), br.supports(n, base, reps + near + [base]))


def test_support_edges_are_checked(hiplib):
    main = br.random_tree_edges(6, np.random.default_rng(0))
    assert (_support(hiplib, 3, (np.array([3, 3, 3]), np.array([0, 1, 2])), [(np.array([3, 3, 3]), np.array([0, 1, 2]))]) == 0).all()
    with pytest.raises(RuntimeError, match="2n - 3 edges"):
        _support(hiplib, 6, main, [(main[0][:-1], main[1][:-1])])
    bad = (main[0].copy(), main[1].copy())
    bad[1][0] = bad[1][1]
    with pytest.raises(RuntimeError, match="not a tree"):
        _support(hiplib, 6, main, [bad])
    swapped = (main[0][::-1].copy(), main[1][::-1].copy())                  # parents before their children
    with pytest.raises(RuntimeError, match="not a tree"):
        _support(hiplib, 6, main, [swapped])


def test_support_of_a_20000_leaf_caterpillar_needs_no_recursion(hiplib):
    n = 20000
    a, b = br.caterpillar_edges(list(range(n))), br.caterpillar_edges(list(range(n))[::-1])
    got = _support(hiplib, n, a, [b, a])
    assert np.array_equal(got, 2 * (a[1] >= n).astype(np.uint32)) and int((a[1] >= n).sum()) == n - 3


def _write(hiplib, tmp_path, names, parent, child, length, support, replicates, ref="r", edges=True):
    out, ed = tmp_path / "t.nwk", tmp_path / "t.csv"
    for p in (out, ed):
        if p.exists():
            p.unlink()
    pa, ch, ln = np.ascontiguousarray(parent, np.uint32), np.ascontiguousarray(child, np.uint32), np.ascontiguousarray(length, np.float64)
    su = np.ascontiguousarray(support, np.uint32)
    cn = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    rc = hiplib.tracs_tree_write_support(cn, len(names), pa.ctypes.data, ch.ctypes.data, ln.ctypes.data, len(pa), su.ctypes.data, replicates,
                                         os.fsencode(str(out)), ref.encode(), os.fsencode(str(ed)) if edges else None)
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


def test_newick_with_support_of_a_small_tree_and_its_edge_rows(hiplib, tmp_path):
    D = np.array([[0, 5, 9, 9, 8], [5, 0, 10, 10, 9], [9, 10, 0, 8, 7], [9, 10, 8, 0, 3], [8, 9, 7, 3, 0]], np.float64)
    names = ["a", "b", "c", "d", "e"]
    parent, child, length = nj_ref.nj(D)
    none = br.NONE
    text, rows = _write(hiplib, tmp_path, names, parent, child, length, [none, none, none, 87, none, none, 100], 100, ref="ref1")
    assert text == "(d:2,e:1,(c:4,(a:2,b:3)87:3)100:2);\n"
    assert rows == "#1,a,2,NA,ref1\n#1,b,3,NA,ref1\n#2,c,4,NA,ref1\n#2,#1,3,87,ref1\n#3,d,2,NA,ref1\n#3,e,1,NA,ref1\n#3,#2,2,100,ref1\n"
    # a support of 0 is a label, "none" is not; a value on a leaf edge is not written
    text, rows = _write(hiplib, tmp_path, names, parent, child, length, [7, 7, 7, 0, 7, 7, none], 8)
    assert text == "(d:2,e:1,(c:4,(a:2,b:3)0:3):2);\n"
    assert [r.split(",")[3] for r in rows.splitlines()] == ["NA", "NA", "NA", "0", "NA", "NA", "NA"]
    # without any support: tracs_tree_write's own line
    text, _ = _write(hiplib, tmp_path, names, parent, child, length, [none] * 7, 8)
    assert text == "(d:2,e:1,(c:4,(a:2,b:3):3):2);\n" == _plain(hiplib, tmp_path, names, parent, child, length)
    with pytest.raises(RuntimeError, match="9 out of 8"):
        _write(hiplib, tmp_path, names, parent, child, length, [none, none, none, 9, none, none, 1], 8)
    # the labelled line parses to the same tree, labels on internal nodes only
    text, _ = _write(hiplib, tmp_path, names, parent, child, length, [none, none, none, 3, none, none, 8], 8)
    nodes = nj_ref.parse_newick(text)
    assert sorted(lab for _, lab, _ in nodes if lab is not None) == sorted(names + ["3", "8"])
    kids = {p for p, _, _ in nodes}
    assert all((k in kids) == (lab in ("3", "8", None)) for k, (_, lab, _) in enumerate(nodes))


def test_small_n_and_quoting_with_support(hiplib, tmp_path):
    e = np.zeros(0)
    assert _write(hiplib, tmp_path, ["only"], e, e, e, e, 4) == ("only;\n", "")
    assert _write(hiplib, tmp_path, ["A", "B"], [0], [1], [7.0], [br.NONE], 4) == ("(A:3.5,B:3.5);\n", "A,B,7,NA,r\n")
    assert _write(hiplib, tmp_path, ["A", "B", "C"], [3, 3, 3], [0, 1, 2], [1.0, 2.0, 4.0], [br.NONE] * 3, 4) == \
        ("(A:1,B:2,C:4);\n", "#1,A,1,NA,r\n#1,B,2,NA,r\n#1,C,4,NA,r\n")
    with pytest.raises(RuntimeError, match="2n - 3 edges"):
        _write(hiplib, tmp_path, ["A", "B", "C"], [3, 3], [0, 1], [1.0, 2.0], [0, 0], 4)
    names = ["plain_1.2-x", "with space", "it's", "a,b", "semi;colon", "(paren)", "[br]", "co:lon", "tab\there"]
    n = len(names)
    parent, child, length = nj_ref.nj(nj_ref.random_tree_metric(n, np.random.default_rng(1))[0])
    support = np.where(child >= n, 5, br.NONE).astype(np.uint32)
    text, _ = _write(hiplib, tmp_path, names, parent, child, length, support, 5)
    for want in ("plain_1.2-x:", "'with space':", "'it''s':", "'a,b':", "'semi;colon':", "'(paren)':", "'[br]':", "'co:lon':", "'tab\there':"):
        assert want in text, want
    assert "'plain" not in text and text.count(")5:") == n - 3
    assert text.replace(")5:", "):") == _plain(hiplib, tmp_path, names, parent, child, length)      # labels aside, the same bytes
