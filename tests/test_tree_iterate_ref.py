"""tests/tree_iterate_ref.py itself (the reference of `--tree-iterate`) and the host side of the new entries: no GPU.

  * on the seeded imports the reference moves the tree, stops on a repeat within three iterations, masks something, and no window of
    any iteration lies within branch_filter_ref.MARGIN of its threshold -- so the GPU tests compare exactly;
  * the ctypes mirrors of tracs_tree_iterate and tracs_tree_iterate_result have the layout a C compiler gives the header's structs;
  * the command line's refusals, before any GPU path;
  * without iterate the handle calls tracs_distance_tree_run with the fields it always had."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import branch_filter_ref as bf
import tree_iterate_ref as ti
from test_tree_changes_cli import _no_gpu, _parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (1, 2, 3)


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_imports_meet_their_conditions(oracle, seed):
    """a seed that misses a condition is replaced, never tolerated"""
    masks = ti.import_case(seed)
    assert masks.shape == (10, 20000) and set(np.unique(masks).tolist()) <= {1, 2, 4, 8}
    assert np.array_equal(masks[2, 7000:7200], masks[7, 7000:7200]) and not np.array_equal(masks[2, :7000], masks[7, :7000])
    r = ti.iterate(masks, 100, oracle)
    t0, t1 = ti.splits(10, *r["trees"][0][:2]), ti.splits(10, *r["trees"][1][:2])
    assert len(t0) == len(t1) == 7 and t0 != t1                                        # T_1 differs from T_0 in topology
    assert r["same_as"] is not None and r["iterations"] <= 3                           # a stop by repeat at k <= 3
    assert all(row[5] > 0 for row in r["rows"][:-1]) and r["rows"][-1][5] is None      # masked cells
    assert r["masked_cells_last"] > 0 and r["mask_work_max"] >= max(row[5] for row in r["rows"][:-1])
    assert r["margin"] > bf.MARGIN, r["margin"]
    assert r["rows"][0][6] is None and r["rows"][-1][7] == r["same_as"] and all(row[7] is None for row in r["rows"][:-1])
    assert r["rows"][1][6] == len(t0 & t1) and r["rows"][-1][6] == 7


def test_the_limit_stops_a_run_that_has_not_repeated(oracle):
    r = ti.iterate(ti.import_case(1), 1, oracle)
    assert (r["iterations"], r["same_as"], len(r["rows"]), len(r["trees"])) == (1, None, 2, 2)
    assert r["rows"][1][5] is None and r["rows"][1][7] is None


def test_masking_starts_from_the_original_and_two_samples_end_on_the_filtered_distance(oracle):
    rng = np.random.default_rng(4)
    L = 3000
    base = rng.integers(0, 4, L)
    seqs = np.stack([base, np.where(rng.random(L) < 0.02, (base + 1) % 4, base)])
    seqs[1, 1000:1040] = (base[1000:1040] + 2) % 4
    masks = (1 << seqs).astype(np.int64)
    masks[0, 5:9] = 15
    r = ti.iterate(masks, 5, oracle)
    assert (r["iterations"], r["same_as"]) == (1, 0)                                   # n < 4: no split, T_1 repeats T_0
    kept = int(r["final"][3].sum())
    assert 0 < kept < r["rows"][0][1] and r["trees"][1][2].tolist() == [float(kept)]
    M = r["M"][1]
    assert np.array_equal(M[0], masks[0]) and ((M[1] == 15) == (masks[1] != M[1])).all()      # below(e) = {1}
    assert r["rows"][0][5] == int((M[1] == 15).sum())
    text = ti.text(masks)
    assert kept == int(oracle.filter_recomb_pairs(text, [0], [1])[0])


def test_below_is_the_side_away_from_the_top_node():
    import fitch_ref as fr
    parent, child = fr.caterpillar(6)
    assert [(int(p), int(c)) for p, c in zip(parent, child)] == [(6, 0), (6, 1), (7, 2), (7, 6), (8, 3), (8, 7), (9, 4), (9, 5), (9, 8)]
    assert ti.below(6, parent, child) == [[0], [1], [2], [0, 1], [3], [0, 1, 2], [4], [5], [0, 1, 2, 3]]
    assert ti.below(2, [0], [1]) == [[1]]


def test_the_ctypes_mirrors_have_the_layout_of_the_header(tmp_path):
    from tracs_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    structs = (("tracs_tree_iterate", _lib.TreeIterate), ("tracs_tree_iterate_result", _lib.TreeIterateResult))
    lines = ['#include <stdio.h>', '#include "tracs_hip.h"', 'int main(void)', '{']
    for cname, cls in structs:
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f, _ in cls._fields_]
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {}
    for cname, cls in structs:
        want[cname] = str(C.sizeof(cls))
        want.update({"%s.%s" % (cname, f): str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert got == want
    assert [f for f, _ in _lib.TreeIterate._fields_] == ["max_iterations", "iterations_path"]
    assert [f for f, _ in _lib.TreeIterateResult._fields_] == ["iterations", "same_as", "masked_cells_last", "mask_work_max"]
    assert len(_lib.TreeRequest._fields_) == 19 and len(_lib.TreeResult._fields_) == 6            # (the request did not grow)


def test_header_binding_list_and_library_have_the_entries(hiplib):
    from tracs_amd import _lib
    header = open(os.path.join(ROOT, "include", "tracs_hip.h")).read()
    for name in ("tracs_alignment_clone", "tracs_alignment_restore", "tracs_alignment_mask_subtrees", "tracs_distance_tree_iterate"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SYMBOLS and hasattr(hiplib, name), name
    for words in ("always from A, never from M_{k-1}", "the side away from T's top node", "Fitch of the ORIGINAL alignment on the final tree",
                  "the message names the iteration"):
        assert words in header, words
    blob = open(_lib.LIB_PATH, "rb").read()
    for kernel in (b"mask_cells_kernel", b"mask_weights_kernel"):
        assert kernel in blob, kernel
    assert hiplib.tracs_abi_version() == 1
    # argument errors need no GPU
    req, it = _lib.TreeRequest(path=b"o.nwk", ref=b"r", changes=1, filter=1), _lib.TreeIterate(3, None)
    res, ires = _lib.TreeResult(*[7] * 6), _lib.TreeIterateResult(7, 7, 7, 7)
    assert hiplib.tracs_distance_tree_iterate(None, C.byref(req), C.byref(it), C.byref(res), C.byref(ires)) == -1
    assert hiplib.tracs_last_error().startswith(b"tracs_distance_tree_iterate:")
    assert [getattr(res, name) for name, _ in res._fields_] == [0] * 6
    assert (ires.iterations, ires.same_as, ires.masked_cells_last, ires.mask_work_max) == (0, -1, 0, 0)
    assert hiplib.tracs_distance_tree_iterate(None, C.byref(req), None, C.byref(res), None) == -1
    assert hiplib.tracs_last_error().startswith(b"tracs_distance_tree_run:")                      # (it == NULL: that function)
    assert hiplib.tracs_alignment_mask_subtrees(None, None, None, 0, None, None, None, 0, None, None) == -1
    assert b"tracs_alignment_mask_subtrees" in hiplib.tracs_last_error()
    assert hiplib.tracs_alignment_clone(None, None, None) == -1
    assert b"tracs_alignment_clone" in hiplib.tracs_last_error()


def test_defaults_off_and_the_help_says_what_the_iteration_is(capsys):
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj"])
    assert a.tree_iterate is None and a.tree_iterate_out is None
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj", "--tree-filter", "--tree-iterate", "4", "--tree-iterate-out", "i.csv"])
    assert (a.tree_iterate, a.tree_iterate_out) == (4, "i.csv")
    with pytest.raises(SystemExit):
        _parser().parse_args(["-h"])
    text = " ".join(capsys.readouterr().out.split()).replace("- ", "-")        # (argparse may wrap at a hyphen)
    for words in ("--tree-iterate K", "--tree-iterate-out FILE", "one Fitch placement among possibly several", "a screen, not a test",
                  "13 %", "away from the tree's top node", "converged, or a cycle"):
        assert words in text, words


REFUSALS = [
    (["--tree-iterate", "3"], ["--tree-iterate", "needs --tree-filter, which needs --tree"]),
    (["--tree-iterate-out", "i.csv"], ["--tree-iterate", "needs --tree-filter, which needs --tree"]),
    (["--tree", "nj", "--tree-iterate", "3"], ["--tree-iterate", "needs --tree-filter"]),
    (["--tree", "nj", "--tree-edges", "e.csv", "--tree-iterate", "3"], ["--tree-iterate", "needs --tree-filter"]),
    (["--tree", "nj", "--tree-filter", "--tree-edges", "e.csv", "--tree-iterate", "0"], ["--tree-iterate 0", "[1, 100]"]),
    (["--tree", "nj", "--tree-filter", "--tree-edges", "e.csv", "--tree-iterate", "101"], ["--tree-iterate 101", "[1, 100]"]),
    (["--tree", "nj", "--tree-filter", "--tree-edges", "e.csv", "--tree-iterate-out", "i.csv"], ["--tree-iterate-out", "needs --tree-iterate"]),
    (["--tree", "nj", "--tree-edges", "e.csv", "--tree-iterate", "3", "--bootstrap", "10"], ["--tree-iterate", "--bootstrap", "cannot be combined"]),
    (["--tree", "nj", "--tree-filter", "--tree-iterate", "3"], ["--tree-filter", "needs --tree-edges, --tree-changes or --tree-filtered"]),
]


@pytest.mark.parametrize("extra,words", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_refusals_before_any_gpu_path(tmp_path, monkeypatch, extra, words):
    _no_gpu(monkeypatch)
    monkeypatch.chdir(tmp_path)
    a = _parser().parse_args(["--msa", "x.fa", "-o", str(tmp_path / "o.nwk")] + extra)
    with pytest.raises(SystemExit) as e:
        a.func(a)
    msg = str(e.value.code)
    assert msg.startswith("tracs distance: ") and "\n" not in msg
    for w in words:
        assert w in msg, (w, msg)
    assert not any(os.path.exists(tmp_path / x) for x in ("o.nwk", "e.csv", "i.csv"))


@pytest.mark.parametrize("clash", ["-o", "--msa", "--tree-edges", "--tree-changes", "--tree-sites", "--tree-filtered"])
def test_tree_iterate_out_must_not_name_another_file_of_the_run(tmp_path, monkeypatch, clash):
    _no_gpu(monkeypatch)
    paths = {"-o": tmp_path / "o.nwk", "--msa": tmp_path / "x.fa", "--tree-edges": tmp_path / "e.csv", "--tree-changes": tmp_path / "c.csv",
             "--tree-sites": tmp_path / "s.csv", "--tree-filtered": tmp_path / "f.nwk"}
    a = _parser().parse_args(["--msa", str(paths["--msa"]), "-o", str(paths["-o"]), "--tree", "nj", "--tree-edges", str(paths["--tree-edges"]),
                              "--tree-changes", str(paths["--tree-changes"]), "--tree-sites", str(paths["--tree-sites"]), "--tree-filter",
                              "--tree-filtered", str(paths["--tree-filtered"]), "--tree-iterate", "2", "--tree-iterate-out", str(paths[clash])])
    with pytest.raises(SystemExit) as e:
        a.func(a)
    assert "--tree-iterate-out" in str(e.value.code) and not any(p.exists() for p in paths.values())


def test_the_handle_keeps_its_call_without_iterate_and_takes_the_new_one_with_it():
    from tracs_amd.handle import DistanceHandle, TreeIterateResult, TreeResult
    calls = []

    class Lib:
        def tracs_distance_tree_run(self, h, req, res):
            q = req._obj
            calls.append(("run", {name: getattr(q, name) for name, _ in q._fields_ if not name.startswith("contig_")}))
            res._obj.n_joins, res._obj.n_kept = 5, 2
            return 0

        def tracs_distance_tree_iterate(self, h, req, it, res, ires):
            q = req._obj
            calls.append(("iterate", {name: getattr(q, name) for name, _ in q._fields_ if not name.startswith("contig_")},
                          it._obj.max_iterations, it._obj.iterations_path))
            res._obj.n_changes, res._obj.n_kept = 9, 4
            ires._obj.iterations, ires._obj.same_as, ires._obj.masked_cells_last, ires._obj.mask_work_max = 3, len(calls) - 3, 11, 12
            return 0
    h = DistanceHandle.__new__(DistanceHandle)
    h.L, h.h = Lib(), None
    assert h.tree("o", "r", edges_path="e", tree_filter=True, filtered_path="f") == TreeResult(5, 0, 0, 0, 2, 0)
    want = {"kind": 0, "path": b"o", "ref": b"r", "edges_path": b"e", "replicates": 0, "seed": 1, "transfer": 0, "replicate_trees_path": None,
            "changes": 1, "changes_path": None, "sites_path": None, "filter": 1, "filtered_path": b"f", "n_contigs": 0, "max_entries": 100000000,
            "n_threads": 0, "create": 1}
    assert calls == [("run", want)]
    assert h.tree("o", "r", edges_path="e", tree_filter=True, filtered_path="f", iterate=7, iterations_path="i") == \
        TreeIterateResult(0, 0, 9, 0, 4, 0, 3, None, 11, 12)                                  # (same_as -1: None)
    assert h.tree("o", "r", edges_path="e", tree_filter=True, filtered_path="f", iterate=100).same_as == 0
    assert calls[1:] == [("iterate", want, 7, b"i"), ("iterate", want, 100, None)]
    for kw, words in ((dict(iterate=3), "iterate needs tree_filter"), (dict(iterations_path="i", tree_filter=True, edges_path="e"), "needs iterate"),
                      (dict(iterate=0, tree_filter=True, edges_path="e"), r"\[1, 100\]"), (dict(iterate=101, tree_filter=True, edges_path="e"), r"\[1, 100\]")):
        with pytest.raises(ValueError, match=words):
            h.tree("o", "r", **kw)
    assert len(calls) == 3


def test_the_sum_line_of_the_stage_trace_names_the_route(monkeypatch):
    """without the new flags `--tree-filter` reports itself as tracs_distance_tree_filter with its kept count, as it always did; the
    iterated run has a line of its own; the changes run and the plain run keep theirs"""
    import contextlib

    import tracs_amd.distance as di
    from tracs_amd.handle import TreeIterateResult, TreeResult

    class Handle:
        def tree(self, *a, **kw):
            return TreeIterateResult(7, 17, 50, 40, 30, 4, 2, 1, 9, 11) if "iterate" in kw else TreeResult(7, 17, 50, 40, 30, 4)

    @contextlib.contextmanager
    def opened(*a, **kw):
        yield Handle()
    monkeypatch.setattr(di, "_opened", opened)
    base = ["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj", "--tree-edges", "e.csv"]
    want = {(): "[sum] tracs_distance_tree (dense panels, joins, tree: 7 joins, 17 edge rows written)",
            ("--tree-sites", "s.csv"): "[sum] tracs_distance_tree_changes (dense panels, joins, tree, Fitch count and fill: 7 joins, 17 edge rows, "
                                       "50 changes)",
            ("--tree-filter",): "[sum] tracs_distance_tree_filter (dense panels, joins, tree, Fitch count, edge lists, filter, fill: 7 joins, "
                                "17 edge rows, 50 changes, 30 kept)",
            ("--tree-filter", "--tree-iterate", "5"): "[sum] tracs_distance_tree_iterate (3 trees: dense panels, joins, Fitch count, edge lists, "
                                                      "filter, mask each; tree, fill: 7 joins, 17 edge rows, 50 changes, 30 kept)"}
    for extra, line in want.items():
        args = _parser().parse_args(base + list(extra))
        args.tree_files_made = False
        seen = []
        di._tree_on_device(["x.fa"], args, None, "x", seen.append)
        assert seen == [line], extra
