"""Transfer bootstrap support on the GPU (csrc/transfer.hip, tracs_distance_tree_bootstrap_transfer) against
tests/transfer_ref.py: transfer_phi_kernel's phi for every internal edge of the main tree, exactly; the state's sums over several
replicates; and `tracs distance --tree nj --bootstrap B --bootstrap-support transfer` end to end, every label bit for bit."""
import argparse
import ctypes as C
import math
import re

import numpy as np
import pytest

import bootstrap_ref as br
import nj_ref
import transfer_ref as tr

pytestmark = pytest.mark.gpu

KEEP = 0xABCD                                                              # what the entries of leaf edges hold before a call


def _phi(hiplib, n, main, rep):
    """tracs_tree_transfer -> list per edge of main, NONE on leaf edges (which the call must leave alone)"""
    p, c = (np.ascontiguousarray(x, np.uint32) for x in main[:2])
    rp, rc = (np.ascontiguousarray(x, np.uint32) for x in rep[:2])
    out = np.full(len(p), KEEP, np.uint32)
    if hiplib.tracs_tree_transfer(n, p.ctypes.data, c.ctypes.data, len(p), rp.ctypes.data, rc.ctypes.data, len(rp), out.ctypes.data):
        raise RuntimeError(hiplib.tracs_last_error().decode())
    assert (out[(c < n) | (n < 4)] == KEEP).all()
    return [int(x) if ch >= n and n >= 4 else tr.NONE for x, ch in zip(out, c)]


@pytest.mark.parametrize("n", [4, 5, 6, 33, 34, 66, 67, 68, 131, 132])
def test_phi_on_random_trees(hiplib, n):
    """n - 3 = 1, 2, 3, 63, 64, 65, 128, 129 lanes (n = 4, 5, 6, 66, 67, 68, 131, 132); 2n - 3 = 63, 65 entries (n = 33, 34)"""
    rng = np.random.default_rng(500 + n)
    main = br.random_tree_edges(n, rng)
    reps = [br.random_tree_edges(n, rng) for _ in range(3)] + [nj_ref.nj(nj_ref.random_tree_metric(n, rng)[0])[:2]]
    for k, rep in enumerate(reps):
        assert _phi(hiplib, n, main, rep) == tr.phi(n, main, rep), (n, k)
    # main = replicate: every split is there
    got = _phi(hiplib, n, main, main)
    assert [x for x in got if x != tr.NONE] == [0] * (n - 3)
    # the main tree with one leaf hung elsewhere: one leaf has to move, at most
    if n >= 5:
        for leaf, where in ((0, 3), (n - 1, 2 * n), (n // 2, 5 * n + 1)):
            rep = tr.rehung(n, main[0], main[1], leaf, where)
            got = _phi(hiplib, n, main, rep)
            assert got == tr.phi(n, main, rep), (n, leaf, where)
            assert max(x for x in got if x != tr.NONE) <= 1


@pytest.mark.parametrize("reverse", [False, True], ids=["ascending", "descending"])
def test_phi_against_a_2000_leaf_caterpillar(hiplib, reverse):
    """a replicate 2 000 nodes high: a stack that followed the tree's height would overflow the kernel's 40 entries; the program's is 3"""
    n = 2000
    main = br.random_tree_edges(n, np.random.default_rng(11))
    order = list(range(n))[::-1] if reverse else list(range(n))
    rep = br.caterpillar_edges(order)
    assert _phi(hiplib, n, main, rep) == tr.phi(n, main, rep)


def test_phi_against_a_balanced_replicate(hiplib):
    """the deepest stack a tree of 256 leaves can ask for; and the balanced tree as the main tree against a caterpillar"""
    n = 256
    bal = tr.balanced_edges(n)
    assert tr.program(n, *bal)[1] >= 8
    main = br.random_tree_edges(n, np.random.default_rng(12))
    assert _phi(hiplib, n, main, bal) == tr.phi(n, main, bal)
    cat = br.caterpillar_edges(list(range(n)))
    assert _phi(hiplib, n, bal, cat) == tr.phi(n, bal, cat)


def test_malformed_trees_are_refused(hiplib):
    main = br.random_tree_edges(6, np.random.default_rng(0))
    bad = (main[0].copy(), main[1].copy())
    bad[1][0] = bad[1][1]
    with pytest.raises(RuntimeError, match="not a tree in creation order"):
        _phi(hiplib, 6, main, bad)
    with pytest.raises(RuntimeError, match="not a tree in creation order"):
        _phi(hiplib, 6, bad, main)
    with pytest.raises(RuntimeError, match="2n - 3 edges"):
        _phi(hiplib, 6, main, (main[0][:-1], main[1][:-1]))


def test_the_state_sums_three_replicates(hiplib):
    import torch
    n = 67                                                                  # 64 lanes: exactly one full wave
    rng = np.random.default_rng(67)
    main = br.random_tree_edges(n, rng)
    reps = [br.random_tree_edges(n, rng), br.caterpillar_edges(list(range(n))[::-1]), tr.rehung(n, main[0], main[1], 5, 17)]
    p, c = (np.ascontiguousarray(x, np.uint32) for x in main)
    ne = len(p)
    state = torch.empty(hiplib.tracs_transfer_state_bytes(n), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    check = lambda rc: rc == 0 or pytest.fail(hiplib.tracs_last_error().decode())      # noqa: E731
    check(hiplib.tracs_transfer_init(state.data_ptr(), n, p.ctypes.data, c.ctypes.data, ne, stream))
    for k, rep in enumerate(reps):
        rp, rc = (np.ascontiguousarray(x, np.uint32) for x in rep)
        phi = torch.full((ne,), KEEP, dtype=torch.int32, device="cuda")
        check(hiplib.tracs_transfer_add(state.data_ptr(), n, rp.ctypes.data, rc.ctypes.data, len(rp), phi.data_ptr() if k != 1 else None, stream))
        torch.cuda.synchronize()
        want = tr.phi(n, main, rep)
        if k != 1:                                                          # the optional per-replicate output
            assert phi.cpu().numpy().tolist() == [KEEP if w == tr.NONE else w for w in want], k
    sums, light = np.full(ne, KEEP, np.uint64), np.full(ne, KEEP, np.uint32)
    check(hiplib.tracs_transfer_emit(state.data_ptr(), n, sums.ctypes.data, light.ctypes.data))
    want_s, want_p, want_x = tr.transfer(n, main, reps)
    assert sums.tolist() == [KEEP if w == tr.NONE64 else w for w in want_s]      # leaf-edge entries untouched
    assert light.tolist() == [KEEP if w == tr.NONE else w for w in want_p]
    # init again: the sums start from zero
    check(hiplib.tracs_transfer_init(state.data_ptr(), n, p.ctypes.data, c.ctypes.data, ne, stream))
    check(hiplib.tracs_transfer_emit(state.data_ptr(), n, sums.ctypes.data, None))
    assert sums[c >= n].tolist() == [0] * (n - 3)
    # a state of another n is refused; n < 4 does nothing
    assert hiplib.tracs_transfer_emit(state.data_ptr(), n + 1, sums.ctypes.data, None) == -1
    three = (np.array([3, 3, 3], np.uint32), np.array([0, 1, 2], np.uint32))
    small = torch.zeros(hiplib.tracs_transfer_state_bytes(3), dtype=torch.uint8, device="cuda")
    check(hiplib.tracs_transfer_init(small.data_ptr(), 3, three[0].ctypes.data, three[1].ctypes.data, 3, stream))
    check(hiplib.tracs_transfer_add(small.data_ptr(), 3, three[0].ctypes.data, three[1].ctypes.data, 3, None, stream))
    s3 = np.full(3, KEEP, np.uint64)
    check(hiplib.tracs_transfer_emit(small.data_ptr(), 3, s3.ctypes.data, None))
    assert s3.tolist() == [KEEP] * 3 and _phi(hiplib, 3, three, three) == [tr.NONE] * 3
    # the Python entry point
    from tracs_amd import api
    got_s, got_p, got_x = api.tree_transfer(n, main, reps)
    assert got_s.tolist() == want_s and got_p.tolist() == want_p
    assert all((math.isnan(w) and math.isnan(g)) or g == w for g, w in zip(got_x.tolist(), want_x))
    assert np.isnan(api.tree_transfer(3, three, [three])[2]).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

B, SEED = 8, 3
LABEL = re.compile(r"\)([0-9][0-9.e+-]*):")


def run_cli(argv):
    from tracs_amd.distance import distance_parser
    a = distance_parser(argparse.ArgumentParser()).parse_args(argv + ["--loglevel", "ERROR"])
    a.func(a)


def write(path, seqs, names=None):
    from tracs_amd import synth
    return synth.write_fasta(str(path), seqs, names=names or ["s%d" % i for i in range(seqs.shape[0])], width=60)


def bootstrap_run(tmp, fa, tag, kind="transfer", extra=()):
    out, ed, trees = tmp / (tag + ".nwk"), tmp / (tag + ".csv"), tmp / (tag + ".trees")
    run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(out), "--bootstrap", str(B), "--bootstrap-seed", str(SEED), "--tree-edges", str(ed),
             "--bootstrap-trees", str(trees)] + (["--bootstrap-support", kind] if kind else []) + list(extra))
    return out.read_text(), ed.read_text(), trees.read_text()


@pytest.fixture(scope="module")
def outbreak():
    """the fixture and its restatement, computed once: seqs, main edges, replicate edges, split counts, (sums, p, x)"""
    seqs = br.outbreak_alignment()
    n = seqs.shape[0]
    main = nj_ref.nj(br.snp_matrix(seqs).astype(np.float64))
    reps = [br.replicate_tree(seqs, SEED, b) for b in range(B)]
    return seqs, main, reps, br.supports(n, main, reps), tr.transfer(n, main, reps)


def check_transfer(newick, rows, names, main, split, x, ref):
    n = len(names)
    parent, child, length = main
    name = lambda v: names[v] if v < n else "#%d" % (v - n + 1)            # noqa: E731
    assert rows[0] == "parent,child,length,support,transfer,MSA file" and rows[-1] == "" and len(rows) == len(parent) + 2
    for row, p, c, ln, s, xe in zip(rows[1:-1], parent.tolist(), child.tolist(), length.tolist(), split.tolist(), x):
        f = row.split(",")
        assert f[:2] == [name(p), name(c)] and float(f[2]) == ln and f[5] == ref, row
        if c < n:
            assert f[3:5] == ["NA", "NA"], row
        else:
            assert f[3] == str(s) and float(f[4]) == xe, (row, s, xe)
    # the labels of the Newick line: the transfer support of the edge above each internal node, found by its split
    nodes = nj_ref.parse_newick(newick)
    index = {nm: k for k, nm in enumerate(names)}
    below = [0] * len(nodes)
    kids = {p for p, _, _ in nodes if p is not None}
    want = {s: x[e] for s, e in br.internal_splits(n, parent, child).items()}
    seen = 0
    for k in range(len(nodes) - 1, 0, -1):
        p, lab, _ = nodes[k]
        if k not in kids:
            below[k] = 1 << index[lab]
        else:
            assert lab is not None and float(lab) == want[nj_ref._norm(below[k], n)], (k, lab)
            seen += 1
        below[p] |= below[k]
    assert seen == n - 3 and nodes[0][1] is None


def test_labels_and_rows_are_the_restatement(hiplib, outbreak, tmp_path):
    seqs, main, reps, split, (sums, p, x) = outbreak
    n = seqs.shape[0]
    assert (int(split[43]), sums[43], p[43], x[43]) == (0, 21, 10, 0.7083333333333333) and x[41] == 0.7727272727272727
    fa = tmp_path / "ref1_combined.fasta"
    names = write(fa, seqs)
    newick, rows, trees = bootstrap_run(tmp_path, fa, "t")
    check_transfer(newick, rows.split("\n"), names, main, split, x, "ref1")
    assert ")0.7083333333333333:" in newick and ",0,0.7083333333333333,ref1\n" in rows and ",8,1,ref1\n" in rows
    # the run without the option: its support column, its replicate trees and (labels aside) its Newick line
    for kind in (None, "split"):
        s_newick, s_rows, s_trees = bootstrap_run(tmp_path, fa, "s", kind=kind)
        assert s_rows.split("\n")[0] == "parent,child,length,support,MSA file"
        assert [r.split(",")[:4] + r.split(",")[5:] for r in rows.split("\n")[1:-1]] == [r.split(",") for r in s_rows.split("\n")[1:-1]]
        assert s_trees == trees and LABEL.sub("):", s_newick) == LABEL.sub("):", newick) != newick
    plain = tmp_path / "plain.nwk"
    run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(plain)])
    assert LABEL.sub("):", newick) == plain.read_text()
    # two runs: identical files
    assert bootstrap_run(tmp_path, fa, "again") == (newick, rows, trees)
    # the Python entry point on the same trees
    from tracs_amd import api
    got = api.tree_transfer(n, main, reps)
    assert got[0].tolist() == sums and got[1].tolist() == p
    assert all((math.isnan(w) and math.isnan(g)) or g == w for g, w in zip(got[2].tolist(), x))


@pytest.mark.parametrize("panel_rows", ["1", "7"])
def test_several_panels_give_identical_files(hiplib, outbreak, tmp_path, monkeypatch, panel_rows):
    fa = tmp_path / "a.fa"
    write(fa, outbreak[0])
    whole = bootstrap_run(tmp_path, fa, "whole")
    monkeypatch.setenv("TRACS_FOREST_PANEL_ROWS", panel_rows)
    assert bootstrap_run(tmp_path, fa, "panels") == whole


def test_rules_give_the_run_on_the_reduced_fasta(hiplib, outbreak, tmp_path):
    """--mask and --max-sample-n-share: every file equals the run on the FASTA with those columns and records deleted"""
    base = outbreak[0]
    n, L = base.shape
    rng = np.random.default_rng(8)
    seqs = np.concatenate([base[:5], base[5:6], base[5:]], axis=0)           # 25 records ...
    seqs[5, rng.random(L) < 0.7] = ord("N")                                 # ... one of them mostly N
    mask = np.zeros(L, bool)
    mask[40:170] = True
    mask[L - 30:] = True
    G = 0.3
    n_count = (br.MASKS[seqs] == 15)[:, ~mask].sum(axis=1)
    kept = n_count <= math.floor(G * int((~mask).sum()))
    assert (~kept).sum() == 1 and not kept[5]
    fa, bed, red = tmp_path / "full.fa", tmp_path / "mask.bed", tmp_path / "full_reduced.fa"
    names = write(fa, seqs, names=["r%d" % i for i in range(n + 1)])
    bed.write_text("chr\t40\t170\nchr\t%d\t%d\n" % (L - 30, L))
    got = bootstrap_run(tmp_path, fa, "ruled", extra=["--mask", str(bed), "--max-sample-n-share", str(G)])
    reduced = np.ascontiguousarray(seqs[kept][:, ~mask])
    left = [nm for nm, k in zip(names, kept) if k]
    write(red, reduced, names=left)
    want = bootstrap_run(tmp_path, red, "reduced")
    assert got[0] == want[0] and got[2] == want[2]
    assert got[1].replace(",full\n", ",X\n") == want[1].replace(",full_reduced\n", ",X\n") and ",full\n" in got[1]
    # and both are the restatement's on the reduced text
    main = nj_ref.nj(br.snp_matrix(reduced).astype(np.float64))
    reps = [br.replicate_tree(reduced, SEED, b) for b in range(B)]
    check_transfer(got[0], got[1].split("\n"), left, main, br.supports(len(left), main, reps), tr.transfer(len(left), main, reps)[2], "full")


def test_fewer_than_four_samples_write_no_labels(hiplib, tmp_path):
    fa = tmp_path / "few.fa"
    for n in (1, 2, 3):
        write(fa, br.outbreak_alignment()[[0, 9, 20][:n]], names=["A", "B", "C"][:n])
        newick, rows, trees = bootstrap_run(tmp_path, fa, "few%d" % n)
        plain = tmp_path / "few.nwk"
        run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(plain)])
        assert newick == plain.read_text() and trees == ""
        rows = rows.split("\n")
        assert rows[0] == "parent,child,length,support,transfer,MSA file" and len(rows) == (2 * n - 3 if n > 1 else 0) + 2
        assert all(r.split(",")[3:5] == ["NA", "NA"] for r in rows[1:-1])
