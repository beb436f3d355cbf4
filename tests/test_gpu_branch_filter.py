"""The branch filter's device stages by exact integer equality: tracs_fitch_edge_sites against fitch_ref's entries
regrouped by edge, tracs_filter_recomb_lists against tests/golden/filter_hp_golden.json (the definition at 50 digits) and, on seeded
lists whose margin tests/test_branch_filter_ref.py checks, against oracle.filter_recomb_positions, and both against the pair filter
on two samples."""
import numpy as np
import pytest

import branch_filter_ref as bf
import fitch_ref as fr
from test_branch_filter_ref import fixture_lists
from test_gpu_fitch import ALIGNMENTS, TREES, _masks, _nj_tree, _packed, _tree

pytestmark = pytest.mark.gpu

NS = [2, 3, 4, 5, 65, 257]
LS = [1, 127, 129, 1000, 2049, 4097]        # 2049, 4097: one site into the second and the third wave chunk of 2 048 sites


def _edge_sites(aln, parent, child, **kw):
    from tracs_amd import device as dev
    edge, _, _, _, total = dev.fitch_count(aln, parent, child)
    off, site = dev.fitch_edge_sites(aln, parent, child, edge, **kw)
    return off.cpu().numpy(), site.cpu().numpy().astype(np.int64), total


def _same_lists(got, lists, what):
    off, site, total = got
    want_off, want_pos = bf.flat(lists)
    assert np.array_equal(off, want_off), (what, "edge_off")
    assert total == want_off[-1] and np.array_equal(site, want_pos), (what, "edge_site")


@pytest.mark.parametrize("n", NS)
def test_edge_lists_equal_the_regrouped_reference(hiplib, monkeypatch, n):
    """every L; over the six lengths each tree meets each kind of alignment; slabs of one group, the default slab, and (on the two
    longest) a matrix of one chunk, which moves the per-edge cursor from range to range"""
    rng = np.random.default_rng(3000 + n)
    for li, L in enumerate(LS):
        for ti, tree in enumerate(TREES):
            kind = ALIGNMENTS[(li * 4 + ti) % 5]
            masks = _masks(kind, n, L, rng)
            aln = _packed(masks)
            parent, child = _tree(tree, aln, rng)
            _, lists = bf.edge_lists(parent, child, masks)
            monkeypatch.setenv("TRACS_FITCH_SLAB_GROUPS", "1")
            _same_lists(_edge_sites(aln, parent, child), lists, (n, L, tree, kind, "slabs of one group"))
            monkeypatch.delenv("TRACS_FITCH_SLAB_GROUPS")
            _same_lists(_edge_sites(aln, parent, child), lists, (n, L, tree, kind, "default slab"))
            if L > 2048:
                monkeypatch.setenv("TRACS_FITCH_MATRIX_CHUNKS", "1")
                _same_lists(_edge_sites(aln, parent, child), lists, (n, L, tree, kind, "one chunk per range"))
                monkeypatch.delenv("TRACS_FITCH_MATRIX_CHUNKS")
            aln.close()


def test_edge_lists_store_nothing_beyond_room(hiplib, monkeypatch):
    import torch
    rng = np.random.default_rng(31)
    n, L = 65, 4097
    masks = _masks("acgt + N", n, L, rng)
    aln = _packed(masks)
    parent, child = fr.random_tree(n, rng)
    _, lists = bf.edge_lists(parent, child, masks)
    want_off, want_pos = bf.flat(lists)
    total = int(want_off[-1])
    assert total > 1000
    for env in ({}, {"TRACS_FITCH_MATRIX_CHUNKS": "1"}, {"TRACS_FITCH_SLAB_GROUPS": "3", "TRACS_FITCH_MATRIX_CHUNKS": "2"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for room in (total, total // 2, 1, 0):
            out = torch.full((total + 64,), -7, dtype=torch.int32, device="cuda")
            off, site, _ = _edge_sites(aln, parent, child, room=room, out=out)
            got = out.cpu().numpy()
            assert np.array_equal(off, want_off), (env, room)
            assert np.array_equal(got[:room], want_pos[:room]) and (got[room:] == -7).all(), (env, room)
        for k in env:
            monkeypatch.delenv(k)
    aln.close()


def test_edge_lists_of_one_sample_and_a_malformed_tree(hiplib):
    import torch
    from tracs_amd import device as dev
    from tracs_amd._lib import TracsError
    aln = _packed(np.array([[1, 15, 3, 8] * 40]))
    e = np.zeros(0, np.uint32)
    off, site = dev.fitch_edge_sites(aln, e, e, torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert off.tolist() == [0] and site.numel() == 0
    aln.close()
    rng = np.random.default_rng(9)
    aln = _packed(_masks("acgt", 6, 200, rng))
    parent, child = fr.random_tree(6, rng)
    edge = dev.fitch_count(aln, parent, child)[0]
    with pytest.raises((TracsError, RuntimeError), match="2n - 3 edges"):
        dev.fitch_edge_sites(aln, parent[:-1], child[:-1], edge)
    aln.close()


# ---- the filter on position lists ----------------------------------------------------------------------------------------------------
def _handle(L):
    from tracs_amd import device as dev
    aln = dev.Alignment(1, L)
    aln.pack(np.full((1, L), ord("A"), np.uint8))
    return aln


def _filter_lists(aln, lists, with_dropped=True):
    import torch
    from tracs_amd import device as dev
    off, pos = bf.flat(lists)
    filt, dropped = dev.filter_recomb_lists(aln, torch.from_numpy(off).cuda(), torch.from_numpy(pos.astype(np.int32)).cuda(), with_dropped)
    return filt.cpu().numpy().astype(np.int64), (dropped.cpu().numpy() if with_dropped else None), off


@pytest.mark.parametrize("table", ["rows", "per-entry sum"])
def test_lists_filter_on_the_pinned_boundary(hiplib, monkeypatch, table):
    """every list of the fixture, all L: all at once, in reverse, and a subset first (the rows are built per call from the d it marks)"""
    if table != "rows":
        monkeypatch.setenv("TRACS_FILTER_TABLE", "0")
    fx = fixture_lists()
    for L in sorted({x[0] for x in fx}):
        mine = [(pos, want) for l, pos, want in fx if l == L]
        aln = _handle(L)
        idx = np.arange(len(mine))
        for order in (idx[1::2], idx[::-1], idx):
            filt, dropped, off = _filter_lists(aln, [mine[i][0] for i in order])
            want = np.array([mine[i][1] for i in order])
            assert np.array_equal(filt, want), (table, L, np.nonzero(filt != want)[0][:8])
            run = np.concatenate([[0], np.cumsum(1 - dropped.astype(np.int64))])
            kept = run[off[1:]] - run[off[:-1]]
            assert set(np.unique(dropped)) <= {0, 1} and np.array_equal(kept, want), (table, L)
        counts_only, none, _ = _filter_lists(aln, [m[0] for m in mine], with_dropped=False)
        assert none is None and np.array_equal(counts_only, [m[1] for m in mine])
        aln.close()


@pytest.fixture(scope="module")
def own_cases(oracle):
    """[(name, L, lists, kept per list, dropped flags)], once"""
    out = []
    for name, L, lists in bf.own_edge_cases():
        keep = [bf.verdicts(x, L, oracle) for x in lists]
        kept = np.array([oracle.filter_recomb_positions(x, L) for x in lists], np.int64)
        assert [int(k.sum()) for k in keep] == kept.tolist()
        out.append((name, L, lists, kept, 1 - np.concatenate(keep).astype(np.int64) if len(lists) else np.zeros(0, np.int64)))
    return out


@pytest.mark.parametrize("table", ["rows", "per-entry sum"])
def test_lists_filter_on_its_own_edges(hiplib, monkeypatch, own_cases, table):
    """empty lists between others, d = 1 and 2, adjacent runs, windows beyond the rows' counts, a list beyond the rows' d next to a
    thousand short ones, both ends of the alignment, L = 1: the kept counts and every entry's verdict"""
    if table != "rows":
        monkeypatch.setenv("TRACS_FILTER_TABLE", "0")
    for name, L, lists, kept, dropped_want in own_cases:
        aln = _handle(L)
        filt, dropped, off = _filter_lists(aln, lists)
        assert np.array_equal(filt, kept), (table, name, np.nonzero(filt != kept)[0][:8])
        assert np.array_equal(dropped.astype(np.int64), dropped_want), (table, name)
        aln.close()


def test_lists_filter_refuses_bad_offsets_before_a_launch(hiplib):
    import torch
    from tracs_amd import device as dev
    from tracs_amd._lib import TracsError
    aln = _handle(1000000)
    pos = torch.arange(0, 40, dtype=torch.int32, device="cuda") * 20000              # (out of sight of each other: every entry is kept)
    for off, words in (([0, 10, 5, 40], "decrease"), ([0, 10, 20, 41], "beyond"), ([1, 10, 20, 40], r"off\[0\]")):
        with pytest.raises((TracsError, RuntimeError), match=words):
            dev.filter_recomb_lists(aln, torch.tensor(off, dtype=torch.int64, device="cuda"), pos)
    filt, dropped = dev.filter_recomb_lists(aln, torch.tensor([0, 10, 20, 40], dtype=torch.int64, device="cuda"), pos)      # and it is fine afterwards
    assert filt.cpu().tolist() == [10, 10, 20] and not dropped.any()
    aln.close()


# ---- it is the same filter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [129, 9000, 120000])
def test_two_samples_the_one_edge_is_the_pair(hiplib, L):
    """the one edge's kept changes = filter_recomb_pairs of the pair (0, 1); and a pair call before and after the branch filter on
    one handle gives the same"""
    import torch
    from tracs_amd import device as dev
    rng = np.random.default_rng(L)
    base = rng.integers(0, 4, L)
    seqs = np.stack([base, np.where(rng.random(L) < 0.02, rng.integers(0, 4, L), base)])
    for start in (L // 3, L // 2):                                                  # two stretches that look imported
        hot = slice(start, start + 30)
        seqs[1, hot] = (seqs[0, hot] + 1) % 4
    masks = np.where(rng.random((2, L)) < 0.1, 15, 1 << seqs).astype(np.int64)
    aln = _packed(masks)
    parent, child, d = _nj_tree(aln)
    rows, cols = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
    dd = d[0, 1].reshape(1).contiguous()
    before = dev.filter_recomb_pairs(aln, rows, cols, dd).cpu().tolist()
    edge = dev.fitch_count(aln, parent, child)[0]
    off, site = dev.fitch_edge_sites(aln, parent, child, edge)
    filt, dropped = dev.filter_recomb_lists(aln, off, site)
    after = dev.filter_recomb_pairs(aln, rows, cols, dd).cpu().tolist()
    assert off.cpu().tolist() == [0, int(dd.item())] and np.array_equal(site.cpu().numpy(), np.flatnonzero((masks[0] & masks[1]) == 0))
    assert filt.cpu().tolist() == before == after
    assert int(dropped.sum().item()) == int(dd.item()) - before[0]
    assert L < 9000 or before[0] < int(dd.item())                                   # (something is dropped: the case says something)
    aln.close()
    # a fresh handle on which the branch filter comes first: the pair call after it builds its lists and agrees
    aln = _packed(masks)
    edge = dev.fitch_count(aln, parent, child)[0]
    off, site = dev.fitch_edge_sites(aln, parent, child, edge)
    first = dev.filter_recomb_lists(aln, off, site)[0].cpu().tolist()
    assert first == before == dev.filter_recomb_pairs(aln, rows, cols, dd).cpu().tolist()
    aln.close()


def test_marked_entries_carry_the_verdicts(hiplib, oracle):
    """bit 8 of fitch_fill's info = the edge list's dropped flag of that (edge, site); the other bits are fitch_fill's"""
    from tracs_amd import device as dev
    masks, parent, child = bf.tree_case()                                           # (an import on one terminal branch)
    L = masks.shape[1]
    aln = _packed(masks)
    r, lists, kept = bf.branch_filter(parent, child, masks, oracle)
    edge, _, _, off_s, total = dev.fitch_count(aln, parent, child)
    off, site = dev.fitch_edge_sites(aln, parent, child, edge)
    filt, dropped = dev.filter_recomb_lists(aln, off, site)
    assert np.array_equal(filt.cpu().numpy(), kept) and int(kept.sum()) < total
    s, e, info = dev.fitch_fill(aln, parent, child, off_s)
    plain = info.clone()
    dev.fitch_mark_dropped(s, e, info, off, site, dropped)
    got, plain = info.cpu().numpy(), plain.cpu().numpy()
    assert np.array_equal(got & 255, plain) and np.array_equal(plain, [x[2] for x in r["entries"]])
    want = {(ee, int(p)): not k for ee, x in enumerate(lists) for p, k in zip(x, bf.verdicts(x, L, oracle))}
    assert [bool(v >> 8) for v in got] == [want[(ee, ss)] for ss, ee, _ in r["entries"]]
    assert int((got >> 8).sum()) == total - int(kept.sum())
    aln.close()
