"""Bootstrap support on the GPU (csrc/bootstrap.hip, tracs_distance_tree_bootstrap) against tests/bootstrap_ref.py:
the weights, the gathered planes byte for byte against a pack of the repeated text, the distances on a gathered handle, and
`tracs distance --tree nj --bootstrap` end to end -- main tree, every replicate's tree and every support, bit for bit."""
import argparse
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import bootstrap_ref as br
import nj_ref

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 70]
LS = [1, 33, 128, 129, 4133]


def _packed(seqs):
    from tracs_amd import device as dev
    a = dev.Alignment(*seqs.shape)
    a.pack(np.ascontiguousarray(seqs))
    return a


def _plane_bytes(aln):
    import torch
    from tracs_amd.multigpu import _DeviceBytes
    torch.cuda.synchronize()
    return torch.as_tensor(_DeviceBytes(aln.planes_ptr(), aln.nbytes), device="cuda").cpu().numpy().copy()


@pytest.mark.parametrize("L", [1, 31, 128, 129, 4133])
def test_weights_equal_the_restatement(hiplib, L):
    from tracs_amd import device as dev
    for seed in (1, 2 ** 64 - 3):
        for b in (0, 7):
            got = dev.bootstrap_weights(L, seed, b).cpu().numpy().view(np.uint32)
            want = br.weights(L, seed, b)
            assert got.shape == (L,) and int(got.sum()) == L
            assert np.array_equal(got.astype(np.int64), want), (L, seed, b)


def _alignment(n, L):
    """partial IUPAC codes, N, lower case and bytes that are no letter; a column of N and a column nobody differs at"""
    from tracs_amd import synth
    seqs = synth.alignment(n, L, seed=7 * n + L, mu_lineage=3e-2, mu_sample=1e-2, p_n=0.05, p_partial=0.05, p_lower=0.03, p_other=0.02)
    seqs[:, L // 2] = ord("N")
    seqs[:, L // 3] = ord("G")
    seqs[::2, L - 1] = ord("R")
    return seqs


def _crafted_weights(L, rng):
    """name -> int64[L]"""
    def one(col, w):
        x = np.zeros(L, np.int64)
        x[col] = w
        return x
    ones = np.ones(L, np.int64)
    out = {"identity": ones, "drawn": br.weights(L, 1, 0), "drawn 7": br.weights(L, 5, 7), "random 0..3": rng.integers(0, 4, L)}
    for w in (1, 127, 128, 129, 300):
        out["one column x %d" % w] = one((2 * L) // 3, w)
    out["the last column x 300"] = one(L - 1, 300)
    out["the first column x 129"] = one(0, 129)
    last2 = ones.copy()
    last2[L - 1] = 2                                                        # (the last column of a partial last group when L % 128 != 0)
    out["the last column twice"] = last2
    k = L // 128 + 1
    to_k = ones.copy()
    to_k[L // 2] += 128 * k - L                                             # the output ends at 128 k ...
    out["ends at 128 k"] = to_k
    to_k1 = to_k.copy()
    to_k1[0] += 1                                                           # ... and at 128 k + 1
    out["ends at 128 k + 1"] = to_k1
    if L > 140:
        gap = np.zeros(L, np.int64)
        gap[[5, 5 + 131, L - 1]] = (3, 2, 1)                                # a run of 130 zero weights between two kept columns
        out["a run of zeros"] = gap
        far = np.zeros(L, np.int64)
        far[[0, L - 1]] = (200, 200)                                        # ... and of L - 2
        out["the two ends"] = far
    if out["random 0..3"].sum() == 0:
        out["random 0..3"][0] = 1
    assert int(to_k.sum()) % 128 == 0 and int(to_k1.sum()) % 128 == 1
    return out


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n", NS)
def test_gathered_planes_byte_for_byte(hiplib, n, L):
    import torch
    from tracs_amd import device as dev
    seqs = _alignment(n, L)
    assert L < 33 or ((br.MASKS[seqs] == 15).any() and np.isin(br.MASKS[seqs], (3, 5, 6, 9, 10, 12)).any())      # N and partial codes
    canon = br.canonical(seqs)
    src = _packed(seqs)
    before = _plane_bytes(src)
    for name, w in _crafted_weights(L, np.random.default_rng(n * L)).items():
        want = br.repeated(canon, w)
        new = dev.gather_sites(src, w if name != "drawn" else dev.bootstrap_weights(L, 1, 0))
        assert (new.n, new.L) == (n, int(w.sum())) == want.shape, name
        text = new.unpack().cpu().numpy()
        assert np.array_equal(text, want), (name, int((text != want).sum()))
        twin = _packed(want)
        a, b = _plane_bytes(new), _plane_bytes(twin)
        assert a.shape == b.shape and new.nbytes == twin.nbytes, name
        assert np.array_equal(a, b), (name, int((a != b).sum()))           # pad samples, tail bits, pad groups, slack and the N plane
        new.close()
        twin.close()
    assert np.array_equal(_plane_bytes(src), before)                        # the source is left as it was
    # both refusals, and a wrong length
    with pytest.raises(RuntimeError, match="no column drawn"):
        dev.gather_sites(src, np.zeros(L, np.int64))
    big = np.zeros(L, np.int64)
    big[0] = 2 ** 32 - 1
    if L > 1:
        big[L - 1] = 1
        with pytest.raises(RuntimeError, match="2\\^32"):
            dev.gather_sites(src, big)
    with pytest.raises(ValueError, match="weights"):
        dev.gather_sites(src, np.ones(L + 1, np.int64))
    torch.cuda.synchronize()
    src.close()


@pytest.mark.parametrize("n,L", [(65, 129), (70, 4133)])
def test_distances_on_a_gathered_handle(hiplib, n, L):
    import torch
    from tracs_amd import device as dev
    seqs = _alignment(n, L)
    src = _packed(seqs)
    iu = np.triu_indices(n, 1)
    for b in (0, 3):
        w = br.weights(L, 11, b)
        new = dev.gather_sites(src, dev.bootstrap_weights(L, 11, b))
        d = torch.full((n, n), -1, dtype=torch.int32, device="cuda")
        nn = torch.full((n, n), -1, dtype=torch.int32, device="cuda")
        dev.pairsnp_dense(new, d, nn)
        torch.cuda.synchronize()
        want = br.snp_matrix(seqs, w)
        assert np.array_equal(d.cpu().numpy().astype(np.int64)[iu], want[iu]), b
        assert np.array_equal(want, br.snp_matrix(br.repeated(seqs, w)))
        assert not np.array_equal(want, br.snp_matrix(seqs))                # a no-op gather cannot pass
        new.close()
    src.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

B, SEED = 8, 3


def run_cli(argv):
    from tracs_amd.distance import distance_parser
    a = distance_parser(argparse.ArgumentParser()).parse_args(argv + ["--loglevel", "ERROR"])
    a.func(a)


def write(path, seqs, names=None):
    from tracs_amd import synth
    return synth.write_fasta(str(path), seqs, names=names or ["s%d" % i for i in range(seqs.shape[0])], width=60)


def bootstrap_run(tmp, fa, tag, extra=(), seed=SEED):
    out, ed, tr = tmp / (tag + ".nwk"), tmp / (tag + ".csv"), tmp / (tag + ".trees")
    run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(out), "--bootstrap", str(B), "--bootstrap-seed", str(seed), "--tree-edges", str(ed),
             "--bootstrap-trees", str(tr)] + list(extra))
    return out.read_text(), ed.read_text(), tr.read_text()


@pytest.fixture(scope="module")
def outbreak():
    """the fixture and its restatement, computed once: seqs, main edges, replicate edges, supports"""
    seqs = br.outbreak_alignment()
    main = nj_ref.nj(br.snp_matrix(seqs).astype(np.float64))
    reps = [br.replicate_tree(seqs, SEED, b) for b in range(B)]
    return seqs, main, reps, br.supports(seqs.shape[0], main, reps)


def check_replicate_lines(text, names, reps):
    lines = text.split("\n")
    assert len(lines) == len(reps) + 1 and lines[-1] == ""
    n = len(names)
    for b, (line, edges) in enumerate(zip(lines, reps)):
        nodes = nj_ref.parse_newick(line)
        got, want = nj_ref.newick_splits(nodes, names), nj_ref.splits_of(n, *edges)
        assert got.keys() == want.keys(), b
        assert got == want, (b, [(k, got[k], want[k]) for k in got if got[k] != want[k]][:5])      # lengths as doubles, bit for bit
        assert all(lab is None or lab in names for _, lab, _ in nodes), b                              # no labels


def check_supports(newick, rows, names, main, support, ref):
    n = len(names)
    parent, child, length = main
    name = lambda v: names[v] if v < n else "#%d" % (v - n + 1)            # noqa: E731
    assert rows[0] == "parent,child,length,support,MSA file" and rows[-1] == "" and len(rows) == len(parent) + 2
    for row, p, c, x, s in zip(rows[1:-1], parent.tolist(), child.tolist(), length.tolist(), support.tolist()):
        f = row.split(",")
        assert f[:2] == [name(p), name(c)] and float(f[2]) == x and f[4] == ref, row
        assert f[3] == ("NA" if c < n else str(s)), (row, s)
    # the labels of the Newick line: the support of the edge above each internal node, found by its split
    nodes = nj_ref.parse_newick(newick)
    index = {nm: k for k, nm in enumerate(names)}
    below = [0] * len(nodes)
    kids = {p for p, _, _ in nodes if p is not None}
    want = {split: int(support[e]) for split, e in br.internal_splits(n, parent, child).items()}
    seen = 0
    for k in range(len(nodes) - 1, 0, -1):
        p, lab, _ = nodes[k]
        if k not in kids:
            below[k] = 1 << index[lab]
        else:
            assert lab is not None and int(lab) == want[nj_ref._norm(below[k], n)], (k, lab)
            seen += 1
        below[p] |= below[k]
    assert seen == n - 3 and nodes[0][1] is None


def test_main_tree_replicates_and_supports(hiplib, outbreak, tmp_path):
    seqs, main, reps, support = outbreak
    n = seqs.shape[0]
    inner = support[main[1] >= n]
    assert (inner == B).any() and ((inner > 0) & (inner < B)).any()          # (the fixture is not degenerate: tests/test_bootstrap_ref.py)
    fa = tmp_path / "ref1_combined.fasta"
    names = write(fa, seqs)
    newick, rows, trees = bootstrap_run(tmp_path, fa, "a")
    # the main Newick without its labels is the --tree nj run of the same input, byte for byte; so are the edge rows without theirs
    plain, plain_ed = tmp_path / "plain.nwk", tmp_path / "plain.csv"
    run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(plain), "--tree-edges", str(plain_ed)])
    nodes = nj_ref.parse_newick(newick)
    stripped = newick
    for lab in sorted({lab for _, lab, _ in nodes if lab is not None and lab not in names}, key=len, reverse=True):
        stripped = stripped.replace(")%s:" % lab, "):")
    assert stripped == plain.read_text() and newick != stripped
    assert [",".join(r.split(",")[:3] + r.split(",")[4:]) for r in rows.split("\n")[:-1]] == plain_ed.read_text().split("\n")[:-1]
    check_replicate_lines(trees, names, reps)
    check_supports(newick, rows.split("\n"), names, main, support, "ref1")
    # the same command twice: identical files; another seed: another replicate
    assert bootstrap_run(tmp_path, fa, "b") == (newick, rows, trees)
    other = bootstrap_run(tmp_path, fa, "c", seed=4)
    assert other[2] != trees and set(other[2].split("\n")) != set(trees.split("\n"))
    # the Python entry points on the same trees
    from tracs_amd import api
    assert np.array_equal(api.tree_support(n, main, reps), support)


def test_the_command_line_itself(hiplib, outbreak, tmp_path):
    """`python -m tracs_amd distance --tree nj --bootstrap 8 --bootstrap-seed 3 ...` in a process of its own: the files of the run above"""
    fa = tmp_path / "ref1_combined.fasta"
    write(fa, outbreak[0])
    want = bootstrap_run(tmp_path, fa, "inproc")
    out, ed, tr = tmp_path / "cli.nwk", tmp_path / "cli.csv", tmp_path / "cli.trees"
    p = subprocess.run([sys.executable, "-m", "tracs_amd", "distance", "--msa", str(fa), "--tree", "nj", "-o", str(out), "--bootstrap", str(B),
                        "--bootstrap-seed", str(SEED), "--tree-edges", str(ed), "--bootstrap-trees", str(tr), "--loglevel", "ERROR"],
                       capture_output=True, text=True, timeout=300, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    assert (out.read_text(), ed.read_text(), tr.read_text()) == want


@pytest.mark.parametrize("rows", ["1", "7"])
def test_several_panels_give_identical_files(hiplib, outbreak, tmp_path, monkeypatch, rows):
    fa = tmp_path / "a.fa"
    write(fa, outbreak[0])
    whole = bootstrap_run(tmp_path, fa, "whole")
    monkeypatch.setenv("TRACS_FOREST_PANEL_ROWS", rows)
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
    kept_samples = n_count <= math.floor(G * int((~mask).sum()))
    assert (~kept_samples).sum() == 1 and not kept_samples[5]
    fa, bed, red = tmp_path / "full.fa", tmp_path / "mask.bed", tmp_path / "full_reduced.fa"
    names = write(fa, seqs, names=["r%d" % i for i in range(n + 1)])
    bed.write_text("chr\t40\t170\nchr\t%d\t%d\n" % (L - 30, L))
    got = bootstrap_run(tmp_path, fa, "ruled", extra=["--mask", str(bed), "--max-sample-n-share", str(G)])
    reduced = np.ascontiguousarray(seqs[kept_samples][:, ~mask])
    left = [nm for nm, k in zip(names, kept_samples) if k]
    write(red, reduced, names=left)
    want = bootstrap_run(tmp_path, red, "reduced")
    assert got[0] == want[0] and got[2] == want[2]
    assert got[1].replace(",full\n", ",X\n") == want[1].replace(",full_reduced\n", ",X\n") and ",full\n" in got[1]
    # and both are the restatement's on the reduced text (another length, so other draws than the unruled run)
    main = nj_ref.nj(br.snp_matrix(reduced).astype(np.float64))
    reps = [br.replicate_tree(reduced, SEED, b) for b in range(B)]
    check_replicate_lines(got[2], left, reps)
    check_supports(got[0], got[1].split("\n"), left, main, br.supports(len(left), main, reps), "full")


def test_no_differing_column_and_fewer_than_four_samples(hiplib, tmp_path):
    # identical samples: every replicate has the zero matrix, whose tree is the main tree's
    seqs = np.tile(np.frombuffer(b"ACGTNRAC" * 20, np.uint8), (6, 1))
    fa = tmp_path / "same.fa"
    names = write(fa, seqs)
    newick, rows, trees = bootstrap_run(tmp_path, fa, "same")
    main = nj_ref.nj(np.zeros((6, 6)))
    check_replicate_lines(trees, names, [main] * B)
    check_supports(newick, rows.split("\n"), names, main, br.supports(6, main, [main] * B), "same")
    assert newick.count(")%d:" % B) == 3
    # one differing column among 160: a replicate that does not draw it has the zero matrix
    seqs = seqs.copy()
    seqs[:3, 100] = ord("T")
    names = write(fa, seqs)
    newick, rows, trees = bootstrap_run(tmp_path, fa, "one")
    main = nj_ref.nj(br.snp_matrix(seqs).astype(np.float64))
    reps = [br.replicate_tree(seqs, SEED, b) for b in range(B)]
    drawn = [int(br.weights(160, SEED, b)[100]) for b in range(B)]
    assert 0 in drawn and any(drawn)                                        # both kinds of replicate occur
    check_replicate_lines(trees, names, reps)
    check_supports(newick, rows.split("\n"), names, main, br.supports(6, main, reps), "same")
    # n < 4: nothing to label, --tree's own line; the edge rows say NA
    for n in (1, 2, 3):
        write(fa, br.outbreak_alignment()[[0, 9, 20][:n]], names=["A", "B", "C"][:n])
        newick, rows, trees = bootstrap_run(tmp_path, fa, "few%d" % n)
        plain = tmp_path / "few.nwk"
        run_cli(["--msa", str(fa), "--tree", "nj", "-o", str(plain)])
        assert newick == plain.read_text() and trees == ""
        assert all(r.split(",")[3] == "NA" for r in rows.split("\n")[1:-1]) and len(rows.split("\n")) == (2 * n - 3 if n > 1 else 0) + 2
