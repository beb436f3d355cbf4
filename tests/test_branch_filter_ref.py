"""tests/branch_filter_ref.py itself (the reference of the branch filter) and the host side of the new entries: no GPU.

  * on the pinned lists of tests/golden/filter_hp_golden.json the reference gives the fixture's counts;
  * on two samples the one edge's kept changes are the pair's filtered distance;
  * no seeded list of the GPU tests has a window within 1e-9 (relative) of its threshold -- the oracle and the device's tail agree
    to 1.6e-10 there, so those tests compare exactly;
  * the header declares the new entries, the binding list has them and the library exports them."""
import json
import os
import re

import numpy as np
import pytest

import branch_filter_ref as bf
import fitch_ref as fr
import hp_filter as H

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRIES = ("tracs_fitch_edge_sites", "tracs_filter_recomb_lists", "tracs_fitch_mark_dropped", "tracs_tree_write_filtered",
               "tracs_distance_tree_filter")


def fixture_lists():
    """[(L, ascending sites, expected kept)]: every case's boundary positions and its two probes"""
    with open(os.path.join(HERE, "golden", "filter_hp_golden.json")) as fh:
        cases = json.load(fh)["cases"]
    out = []
    for c in cases:
        L, d = c["L"], c["d"]
        out.append((L, np.asarray(H.boundary_positions(L, d, c["row"]), np.int64), c["expected"]))
        shape, at_wh, beyond = c["probe"]
        out.append((L, np.asarray(H.probe_positions(L, d, shape, c["wh"]), np.int64), at_wh))
        out.append((L, np.asarray(H.probe_positions(L, d, shape, c["wh"] + 1), np.int64), beyond))
    return out


def test_reference_gives_the_pinned_counts(oracle):
    lists = fixture_lists()
    assert len(lists) == 75 and len({L for L, _, _ in lists}) >= 2
    for L, pos, want in lists:
        assert oracle.filter_recomb_positions(pos, L) == want, (L, len(pos))
        keep = bf.verdicts(pos, L, oracle)
        assert int(keep.sum()) == want, (L, len(pos))


@pytest.mark.parametrize("kind", ["acgt", "acgt + N"])
def test_two_samples_one_edge_is_the_pair(oracle, kind):
    some_dropped = False
    for L, mu, seed in ((129, 0.2, 1), (2000, 0.05, 2), (9000, 0.01, 3)):
        rng = np.random.default_rng(seed)
        base = rng.integers(0, 4, L)
        seqs = np.stack([base, np.where(rng.random(L) < mu, rng.integers(0, 4, L), base)])
        hot = slice(L // 3, L // 3 + 40)                           # a stretch that looks imported
        seqs[1, hot] = (seqs[0, hot] + 1 + np.arange(40) % 2) % 4
        masks = (1 << seqs).astype(np.int64)
        if kind == "acgt + N":
            masks = np.where(rng.random((2, L)) < 0.2, 15, masks)
        parent, child = fr.tree_from_joins(2, [], [])
        r, lists, kept = bf.branch_filter(parent, child, masks, oracle)
        text = np.frombuffer(fr.LETTERS.encode(), np.uint8)[masks]
        want = oracle.filter_recomb_pairs(text, [0], [1])
        assert len(lists) == 1 and r["total"] == len(lists[0]) == int(((masks[0] & masks[1]) == 0).sum())
        assert kept[0] == int(want[0]), (L, kind)
        some_dropped |= bool(kept[0] < r["total"])
    assert some_dropped                                           # (the stretch is dropped somewhere: the cases say something)


def test_regrouped_entries_are_ascending_and_complete():
    rng = np.random.default_rng(5)
    masks = rng.integers(1, 16, (7, 300))
    parent, child = fr.random_tree(7, rng)
    r, lists = bf.edge_lists(parent, child, masks)
    assert [len(x) for x in lists] == r["edge_changes"].tolist() and sum(len(x) for x in lists) == r["total"]
    for x in lists:
        assert (np.diff(x) > 0).all()
    off, pos = bf.flat(lists)
    assert off[-1] == r["total"] == len(pos)


def test_margin_of_the_seeded_lists(oracle):
    """every list the GPU tests give to filter_recomb_lists: no window within 1e-9 of its threshold, and the per-entry restatement
    agrees with the oracle's count"""
    names = []
    for name, L, lists in bf.own_edge_cases():
        names.append(name)
        for x in lists:
            assert len(x) == 0 or ((np.diff(x) > 0).all() and x[0] >= 0 and x[-1] < L), name
            m = bf.margin(x, L, oracle)
            assert m > bf.MARGIN, (name, len(x), m)
            assert int(bf.verdicts(x, L, oracle).sum()) == oracle.filter_recomb_positions(x, L), (name, len(x))
    assert len(names) == 6
    # the cases hold what they are named for
    by = {name: (L, lists) for name, L, lists in bf.own_edge_cases()}
    L, lists = by["a window with more than 63 changes"]
    assert max(int(bf.windows(x, L)[0].max()) for x in lists) >= 64
    L, lists = by["runs of adjacent sites"]
    assert any(((c > 1) & (c >= n)).any() for c, n in (bf.windows(x, L) for x in lists))
    L, lists = by["70 000 entries next to 1 000 lists of 3"]
    assert sorted({len(x) for x in lists}) == [3, 70000] and len(lists) == 1001
    assert any(not bf.verdicts(x, L, oracle).all() for _, L, ls in bf.own_edge_cases() for x in ls)
    masks, parent, child = bf.tree_case()
    r, lists, kept = bf.branch_filter(parent, child, masks, oracle)
    assert min(bf.margin(x, masks.shape[1], oracle) for x in lists) > bf.MARGIN
    assert 0 < int(kept.sum()) < r["total"] and int((kept < r["edge_changes"]).sum()) >= 1


def test_header_binding_list_and_library_have_the_entries(hiplib):
    from tracs_amd import _lib
    header = open(os.path.join(os.path.dirname(HERE), "include", "tracs_hip.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SYMBOLS and hasattr(hiplib, name), name
    for words in ("DROPPED iff", "0.05 / d_e", "clamp(int(1 / p / 2 + 1), 50, 5000)", "An N leaf never carries a change",
                  "MUST be ascending and below L"):
        assert words in header, words
    m = re.search(r"int tracs_filter_recomb_lists\(([^;]*)\);", header)
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["a", "off", "pos", "n_lists", "n_entries", "filt", "dropped", "stream"]
    blob = open(_lib.LIB_PATH, "rb").read()
    for kernel in (b"flt_lists_kernel", b"fitch_edge_scan_kernel", b"fitch_mark_kernel"):
        assert kernel in blob, kernel
    # argument errors need no GPU
    assert hiplib.tracs_distance_tree_filter(None, 0, b"x", b"r", None, None, None, None, None, None, 0, 1, 1, 1, None, None, None, None, None,
                                             None) == -1
    assert b"tracs_distance_tree_filter" in hiplib.tracs_last_error()
    assert hiplib.tracs_filter_recomb_lists(None, None, None, 3, 0, None, None, None) == -1
    assert b"tracs_filter_recomb_lists" in hiplib.tracs_last_error()
