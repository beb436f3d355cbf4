"""Small parsimony on the GPU (csrc/fitch.hip, tracs_fitch_count / _fill) against tests/fitch_ref.py: the edges'
and the sites' change counts, the minimum, the offsets, the total and every entry, by exact integer equality."""
import numpy as np
import pytest

import fitch_ref as fr

pytestmark = pytest.mark.gpu

NS = [2, 3, 4, 5, 63, 64, 65, 257]          # 65: n_pad = 128, so pad samples; 257: more than one 64-sample tile of the leaves kernel
LS = [1, 127, 128, 129, 1000, 4097]         # tail bits and group edges; with slabs of one group the longer ones cross slabs
TREES = ["nj", "caterpillar", "balanced", "random"]
ALIGNMENTS = ["acgt", "acgt + N", "all 15 masks", "constant", "all N"]


def _masks(kind, n, L, rng):
    if kind == "all 15 masks":
        return rng.integers(1, 16, (n, L))
    if kind == "constant":
        return np.full((n, L), 4, np.int64)
    if kind == "all N":
        return np.full((n, L), 15, np.int64)
    base = rng.integers(0, 4, L)                                           # ACGT only, mu ~ 0.05 around a few lineages
    lineage = np.where(rng.random((4, L)) < 0.05, rng.integers(0, 4, (4, L)), base)
    seqs = lineage[rng.integers(0, 4, n)]
    seqs = np.where(rng.random((n, L)) < 0.05, rng.integers(0, 4, (n, L)), seqs)
    masks = 1 << seqs
    if kind == "acgt + N":
        masks = np.where(rng.random((n, L)) < 0.3, 15, masks)
    return masks.astype(np.int64)


def _packed(masks):
    from tracs_amd import device as dev
    text = np.frombuffer(fr.LETTERS.encode(), np.uint8)[masks]
    a = dev.Alignment(*masks.shape)
    a.pack(np.ascontiguousarray(text))
    return a


def _nj_tree(aln):
    import torch
    from tracs_amd import device as dev
    n = aln.n
    d = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    nn = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    dev.pairsnp_dense(aln, d, nn)
    state = dev.nj_init(n)
    dev.nj_load_panel(state, n, d, nn)
    dev.nj_run(state, n)
    parent, child, _ = dev.nj_edges(n, *dev.nj_emit(state, n))
    return parent, child, d


def _tree(kind, aln, rng):
    n = aln.n
    if kind == "nj":
        return _nj_tree(aln)[:2]
    return {"caterpillar": fr.caterpillar, "balanced": fr.balanced}[kind](n) if kind != "random" else fr.random_tree(n, rng)


def _run(aln, parent, child):
    """count, then one fill -> the reference's dict, from the device"""
    from tracs_amd import device as dev
    edge, site, minimum, off, total = dev.fitch_count(aln, parent, child)
    s, e, info = dev.fitch_fill(aln, parent, child, off)
    return {"edge_changes": edge.cpu().numpy().view(np.uint32).astype(np.int64), "site_changes": site.cpu().numpy().view(np.uint32).astype(np.int64),
            "site_minimum": minimum.cpu().numpy().astype(np.int64), "off": off.cpu().numpy(), "total": total,
            "entries": list(zip(s.cpu().tolist(), e.cpu().tolist(), info.cpu().tolist()))}, off


def _same(got, want, what):
    for key in ("edge_changes", "site_changes", "site_minimum", "off"):
        assert np.array_equal(got[key], want[key]), (what, key)
    assert got["total"] == want["total"] == int(got["edge_changes"].sum()) == int(got["site_changes"].sum()), what
    assert got["entries"] == want["entries"], what


@pytest.mark.parametrize("n", NS)
def test_counts_and_entries_equal_the_definition(hiplib, monkeypatch, n):
    """every L; over the six lengths each tree meets each kind of alignment (4 and 5 are coprime); slabs of one group"""
    monkeypatch.setenv("TRACS_FITCH_SLAB_GROUPS", "1")
    rng = np.random.default_rng(1000 + n)
    for li, L in enumerate(LS):
        for ti, tree in enumerate(TREES):
            kind = ALIGNMENTS[(li * 4 + ti) % 5]
            masks = _masks(kind, n, L, rng)
            aln = _packed(masks)
            parent, child = _tree(tree, aln, rng)
            want = fr.fitch(parent, child, masks)
            assert np.array_equal(want["site_changes"], want["site_cost"])
            got, _ = _run(aln, parent, child)
            _same(got, want, (n, L, tree, kind))
            if kind in ("constant", "all N"):
                assert got["total"] == 0
            aln.close()


@pytest.mark.parametrize("n,L", [(5, 4097), (65, 1000), (257, 4097)])
def test_the_default_slab_gives_the_same(hiplib, monkeypatch, n, L):
    rng = np.random.default_rng(n + L)
    masks = _masks("all 15 masks", n, L, rng)
    aln = _packed(masks)
    parent, child = fr.random_tree(n, rng)
    want = fr.fitch(parent, child, masks)
    monkeypatch.delenv("TRACS_FITCH_SLAB_GROUPS", raising=False)
    _same(_run(aln, parent, child)[0], want, "default slab")
    monkeypatch.setenv("TRACS_FITCH_SLAB_GROUPS", "3")
    _same(_run(aln, parent, child)[0], want, "slabs of three groups")
    aln.close()


@pytest.mark.parametrize("L", [1, 129, 1000])
def test_two_samples_total_is_their_snp_distance(hiplib, L):
    rng = np.random.default_rng(L)
    masks = _masks("all 15 masks", 2, L, rng)
    aln = _packed(masks)
    parent, child, d = _nj_tree(aln)
    assert (list(parent), list(child)) == ([0], [1])
    got, _ = _run(aln, parent, child)
    assert got["total"] == int(d[0, 1].item()) == int(((masks[0] & masks[1]) == 0).sum())
    aln.close()


def test_one_sample_has_no_edge_and_no_change(hiplib):
    masks = np.array([[1, 15, 3, 8] * 40])
    aln = _packed(masks)
    e = np.zeros(0, np.uint32)
    got, _ = _run(aln, e, e)
    _same(got, fr.fitch(e, e, masks), "n = 1")
    assert got["total"] == 0 and not got["site_minimum"].any()
    aln.close()


def test_fill_in_two_ranges_and_nothing_beyond_room(hiplib, monkeypatch):
    import torch
    from tracs_amd import device as dev
    monkeypatch.setenv("TRACS_FITCH_SLAB_GROUPS", "2")
    rng = np.random.default_rng(3)
    n, L = 65, 1000
    masks = _masks("acgt + N", n, L, rng)
    aln = _packed(masks)
    parent, child = fr.random_tree(n, rng)
    want = fr.fitch(parent, child, masks)
    edge, site, minimum, off, total = dev.fitch_count(aln, parent, child)
    assert total == want["total"] > 100
    whole = [t.cpu().numpy() for t in dev.fitch_fill(aln, parent, child, off)]
    cut = 333                                                               # (inside a word)
    a = [t.cpu().numpy() for t in dev.fitch_fill(aln, parent, child, off, 0, cut)]
    b = [t.cpu().numpy() for t in dev.fitch_fill(aln, parent, child, off, cut, L)]
    assert len(a[0]) == want["off"][cut] and len(b[0]) == total - want["off"][cut]
    for k in range(3):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k])
    # both ranges into one pair of buffers under entry_base = 0: the same again
    out = tuple(torch.full((total,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    dev.fitch_fill(aln, parent, child, off, 0, cut, entry_base=0, room=total, out=out)
    dev.fitch_fill(aln, parent, child, off, cut, L, entry_base=0, room=total, out=out)
    for k in range(3):
        assert np.array_equal(out[k].cpu().numpy(), whole[k])
    # a poisoned tail: room is smaller than what the sites hold, and nothing is written at or beyond it
    room = total // 2
    out = tuple(torch.full((total + 64,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    dev.fitch_fill(aln, parent, child, off, 0, L, entry_base=0, room=room, out=out)
    for k in range(3):
        got = out[k].cpu().numpy()
        assert np.array_equal(got[:room], whole[k][:room]) and (got[room:] == -7).all()
    # an entry_base in the middle: the entries before it are left out, not written at negative places
    base = int(want["off"][cut]) + 5
    out = tuple(torch.full((total,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    dev.fitch_fill(aln, parent, child, off, 0, L, entry_base=base, room=total - base, out=out)
    for k in range(3):
        got = out[k].cpu().numpy()
        assert np.array_equal(got[:total - base], whole[k][base:]) and (got[total - base:] == -7).all()
    aln.close()


def test_a_malformed_tree_is_refused_before_a_launch(hiplib):
    from tracs_amd import device as dev
    from tracs_amd._lib import TracsError
    rng = np.random.default_rng(9)
    n = 6
    aln = _packed(_masks("acgt", n, 200, rng))
    parent, child = fr.random_tree(n, rng)

    def refused(p, c, words):
        with pytest.raises((TracsError, RuntimeError), match=words):
            dev.fitch_count(aln, p, c)
    refused(parent[:-1], child[:-1], "2n - 3 edges")
    p, c = parent.copy(), child.copy()
    p[[0, 2]], c[[0, 2]] = p[[2, 0]], c[[2, 0]]                             # an edge out of order
    refused(p, c, "not a tree in creation order")
    p, c = parent.copy(), child.copy()
    c[0], c[1] = c[1], c[0]                                                 # a_t > b_t
    refused(p, c, "not a tree in creation order")
    c = child.copy()
    c[1] = n + 2                                                            # a child id >= its parent (node n)
    refused(parent, c, "not a tree in creation order")
    c = child.copy()
    c[2] = c[0]                                                             # a node that hangs twice
    refused(parent, c, "not a tree in creation order")
    p = parent.copy()
    p[-1] = 2 * n - 4                                                       # the top node is 2n - 3
    refused(p, child, "not a tree in creation order")
    edge, site, minimum, off, total = dev.fitch_count(aln, parent, child)   # and the handle is fine afterwards
    assert total == fr.fitch(parent, child, _masks("acgt", n, 200, np.random.default_rng(9)))["total"]
    aln.close()
