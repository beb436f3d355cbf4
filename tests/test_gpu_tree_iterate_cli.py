"""`tracs distance --tree nj --tree-filter --tree-iterate K --tree-iterate-out FILE` end to end: two --msa files
appended to one set of files under one header each, all six files against tests/tree_iterate_ref.py, a run under --mask, and the run
without the new flags against the reference's first tree."""
import contextlib
import io

import numpy as np
import pytest

import branch_filter_ref as bf
import tree_iterate_ref as ti
from test_gpu_tree_changes_cli import run_cli
from test_gpu_tree_iterate import HEADERS, reference

pytestmark = pytest.mark.gpu

K = 6
FILES = ("t.nwk", "e.csv", "c.csv", "s.csv", "f.nwk", "i.csv")


def _flags(f):
    return ["--tree", "nj", "-o", str(f["t.nwk"]), "--tree-filter", "--tree-edges", str(f["e.csv"]), "--tree-changes", str(f["c.csv"]),
            "--tree-sites", str(f["s.csv"]), "--tree-filtered", str(f["f.nwk"])]


@pytest.fixture(scope="module")
def run(tmp_path_factory, hiplib):
    d = tmp_path_factory.mktemp("tree_iterate")
    cases = {"imp1": reference("import", 1, 0, K), "rnd9": reference("random", 9, 300, K)}
    assert all(r["margin"] > bf.MARGIN for _, r in cases.values())
    msas = []
    for ref, (masks, _) in cases.items():
        fa = d / (ref + "_combined.fasta")
        ti.write_fasta(str(fa), masks)
        msas.append(str(fa))
    f = {k: d / k for k in FILES}
    plain = {k: d / ("plain_" + k) for k in FILES[:5]}
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        run_cli(["--msa"] + msas + _flags(f) + ["--tree-iterate", str(K), "--tree-iterate-out", str(f["i.csv"])])
    run_cli(["--msa"] + msas + _flags(plain))
    return {"dir": d, "cases": cases, "msas": msas, "files": f, "plain": plain, "stderr": err.getvalue()}


def _check(f, ref, k, masks, r, iterations=True):
    names = ["s%d" % i for i in range(masks.shape[0])]
    ti.check_outputs(r, names, ref, f["t.nwk"].read_text().split("\n")[k], ti.rows_of(f["e.csv"], ref, HEADERS["e"]),
                     ti.rows_of(f["c.csv"], ref, HEADERS["c"]), ti.rows_of(f["s.csv"], ref, HEADERS["s"]), f["f.nwk"].read_text().split("\n")[k],
                     ti.rows_of(f["i.csv"], ref, HEADERS["i"]) if iterations else None)


def test_all_six_files_equal_the_reference_under_one_header_each(run):
    f = run["files"]
    for k, (ref, (masks, r)) in enumerate(run["cases"].items()):
        _check(f, ref, k, masks, r)
    assert f["t.nwk"].read_text().count("\n") == f["f.nwk"].read_text().count("\n") == 2
    # the rows of the second file follow the first's
    refs = [ln.rsplit(",", 1)[1] for ln in f["i.csv"].read_text().split("\n")[1:-1]]
    assert refs == sorted(refs) and set(refs) == {"imp1", "rnd9"}


def test_stderr_says_how_the_run_ended(run):
    for ref, (_, r) in run["cases"].items():
        fit, _, _, kept = r["final"]
        how = ("stopped at the limit" if r["same_as"] is None else "converged" if r["same_as"] == r["iterations"] - 1 else
               "cycle back to %d" % r["same_as"])
        line = "tracs distance: %s: tree iterate: %d trees built, %s; final tree: %d changes, %d kept, %d dropped\n" % (
            ref, r["iterations"] + 1, how, fit["total"], int(kept.sum()), fit["total"] - int(kept.sum()))
        assert line in run["stderr"], (line, run["stderr"])
    assert run["cases"]["imp1"][1]["same_as"] == run["cases"]["imp1"][1]["iterations"] - 1          # (the import converges)


def test_without_the_new_flags_the_files_are_the_first_trees(run, oracle):
    """--tree-filter alone: T_0 and V(T_0), as before the iteration existed"""
    for k, (ref, (masks, r)) in enumerate(run["cases"].items()):
        first = {"trees": r["trees"][:1], "final": ti.filtered(*r["trees"][0][:2], masks, oracle)}
        _check(dict(run["plain"], **{"i.csv": None}), ref, k, masks, first, iterations=False)
    assert run["plain"]["t.nwk"].read_bytes() != run["files"]["t.nwk"].read_bytes()                   # (the iteration moved the tree)


def test_a_run_under_a_mask(run, oracle, tmp_path):
    """--mask deletes columns before anything else: the reference on the kept columns; positions are the files'"""
    masks, _ = run["cases"]["imp1"]
    L = masks.shape[1]
    bed, fa = tmp_path / "mask.bed", tmp_path / "ref.fa"
    bed.write_text("chr1\t100\t160\nchr1\t7050\t7060\n")
    fa.write_text(">chr1\n" + "A" * L + "\n")
    keep = np.ones(L, bool)
    keep[100:160] = keep[7050:7060] = False
    r = ti.iterate(masks[:, keep], K, oracle)
    assert r["margin"] > bf.MARGIN
    f = {k: tmp_path / k for k in FILES}
    run_cli(["--msa", run["msas"][0]] + _flags(f) + ["--tree-iterate", str(K), "--tree-iterate-out", str(f["i.csv"]), "--mask", str(bed),
                                                     "--mask-reference", str(fa)])
    names = ["s%d" % i for i in range(masks.shape[0])]
    ti.check_outputs(r, names, "imp1", f["t.nwk"].read_text().split("\n")[0], ti.rows_of(f["e.csv"], "imp1", HEADERS["e"]), None, None,
                     f["f.nwk"].read_text().split("\n")[0], ti.rows_of(f["i.csv"], "imp1", HEADERS["i"]))
    # the change rows are the reference's entries at the kept columns' own positions in the file
    cols = np.flatnonzero(keep)
    fit = r["final"][0]
    got = [(int(x.split(",")[3]), x.split(",")[2]) for x in ti.rows_of(f["c.csv"], "imp1", HEADERS["c"])]
    assert got == [(int(cols[s]), "chr1") for s, _, _ in fit["entries"]]
