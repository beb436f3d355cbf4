"""tracs_alignment_mask_subtrees and tracs_alignment_clone on the GPU (csrc/tree_mask.hip) against numpy: the masked
handle's text through tracs_alignment_unpack, its plane bytes (pad samples, tail bits, pad groups) against a fresh pack of the
reference's text, the count of newly masked cells, the refusals before a launch, and the per-pack caches across a mask."""
import numpy as np
import pytest

import fitch_ref as fr
import tree_iterate_ref as ti

pytestmark = pytest.mark.gpu

NS = [2, 3, 4, 9, 65, 130]                  # 65 and 130: either side of n_pad = 128, so pad samples
LS = [1, 127, 128, 129, 6000]               # tail bits and group edges
TREES = ["caterpillar", "balanced", "random"]
DROPS = ["none", "all", "random"]
FIXED = (0, 31, 32, 127, 128)               # sites every edge lists (those below L, and L - 1): word and group edges


def _packed(masks):
    from tracs_amd import device as dev
    a = dev.Alignment(*masks.shape)
    a.pack(ti.text(masks))
    return a


def _plane_bytes(aln):
    import torch
    from tracs_amd.multigpu import _DeviceBytes
    torch.cuda.synchronize()
    return torch.as_tensor(_DeviceBytes(aln.planes_ptr(), aln.nbytes), device="cuda").cpu().numpy().copy()


def _masks(n, L, rng):
    """ACGT around a base sequence, with N and partial IUPAC codes already present"""
    base = rng.integers(0, 4, L)
    seqs = np.where(rng.random((n, L)) < 0.1, rng.integers(0, 4, (n, L)), base)
    masks = (1 << seqs).astype(np.int64)
    masks = np.where(rng.random((n, L)) < 0.1, 15, masks)
    return np.where(rng.random((n, L)) < 0.05, rng.integers(1, 16, (n, L)), masks).astype(np.int64)


def _tree(kind, n, rng):
    return {"caterpillar": fr.caterpillar, "balanced": fr.balanced}[kind](n) if kind != "random" else fr.random_tree(n, rng)


def _lists(n_edges, L, drop, rng):
    """per edge an ascending list of sites -- the fixed sites and a few random ones -- and its verdicts (kept?)"""
    fixed = sorted({s for s in FIXED + (L - 1,) if s < L})
    lists, keep = [], []
    for e in range(n_edges):
        extra = rng.choice(L, min(L, 12), replace=False) if e % 4 != 3 else np.zeros(0, np.int64)      # (every fourth edge: the fixed sites only)
        sites = np.unique(np.concatenate([np.asarray(fixed, np.int64), extra])) if e % 7 != 5 else np.zeros(0, np.int64)      # (and empty lists)
        lists.append(sites.astype(np.int64))
        keep.append(np.ones(len(sites), bool) if drop == "none" else np.zeros(len(sites), bool) if drop == "all" else rng.random(len(sites)) < 0.5)
    return lists, keep


def _device_lists(lists, keep):
    import torch
    import branch_filter_ref as bf
    off, pos = bf.flat(lists)
    dropped = ~np.concatenate(keep) if len(pos) else np.zeros(0, bool)
    return (torch.from_numpy(off).cuda(), torch.from_numpy(pos.astype(np.int32)).cuda() if len(pos) else torch.zeros(0, dtype=torch.int32, device="cuda"),
            torch.from_numpy(dropped.astype(np.uint8)).cuda() if len(pos) else torch.zeros(0, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("n", NS)
def test_masked_cells_text_and_planes_equal_the_definition(hiplib, n):
    """every L; over the five lengths each tree meets each kind of verdicts (3 and 3 with a shift).  With everything dropped an edge and
    all its ancestors drop the fixed sites together, so cells are offered more than once and must be counted once."""
    from tracs_amd import device as dev
    rng = np.random.default_rng(7000 + n)
    for li, L in enumerate(LS):
        for ti_, tree in enumerate(TREES):
            drop = DROPS[(li + ti_) % 3]
            masks = _masks(n, L, rng)
            parent, child = _tree(tree, n, rng)
            lists, keep = _lists(len(parent), L, drop, rng)
            want, cells, work = ti.mask(masks, parent, child, lists, keep)
            src = _packed(masks)
            before = _plane_bytes(src)
            aln = dev.clone_alignment(src)
            assert (aln.n, aln.L, aln.nbytes) == (n, L, src.nbytes) and aln.planes_ptr() != src.planes_ptr()
            assert np.array_equal(_plane_bytes(aln), before), (n, L, "clone")
            got = dev.mask_subtrees(aln, parent, child, *_device_lists(lists, keep))
            what = (n, L, tree, drop)
            assert got == cells, what
            assert drop != "none" or cells == 0, what
            assert np.array_equal(aln.unpack().cpu().numpy(), ti.text(want)), what
            twin = _packed(want)
            assert np.array_equal(_plane_bytes(aln), _plane_bytes(twin)), what          # pad samples, tail bits and pad groups included
            assert np.array_equal(_plane_bytes(src), before), what                       # the source of the clone is left as it was
            dev.restore_alignment(aln, src)
            assert np.array_equal(_plane_bytes(aln), before), what                       # and gives the clone its bytes back
            if drop == "all" and n >= 4:
                assert work > cells                                                      # (an edge and its ancestor at one site: offered twice)
            for a in (twin, aln, src):
                a.close()


@pytest.mark.parametrize("cells_per_launch", [1, 100, 256, 4096])
def test_the_work_is_run_over_in_ranges(hiplib, monkeypatch, cells_per_launch):
    """TRACS_MASK_RANGE cuts W into launches of that many cells (the default, 2^30, is what W of several 10^9 crosses): every range
    starts where the one before ended, whether or not that is a multiple of the workgroup; the result is that of one launch"""
    from tracs_amd import device as dev
    rng = np.random.default_rng(41)
    n, L = (9, 129) if cells_per_launch == 1 else (130, 6000)
    masks = _masks(n, L, rng)
    parent, child = fr.caterpillar(n)                                                # (deep: W is many times the entries)
    lists, keep = _lists(len(parent), L, "random", rng)
    want, cells, work = ti.mask(masks, parent, child, lists, keep)
    assert work > 3 * cells_per_launch and work > cells > 0                    # (several ranges; cells offered more than once)
    aln = _packed(masks)
    monkeypatch.setenv("TRACS_MASK_RANGE", str(cells_per_launch))
    assert dev.mask_subtrees(aln, parent, child, *_device_lists(lists, keep)) == cells
    monkeypatch.delenv("TRACS_MASK_RANGE")
    assert np.array_equal(aln.unpack().cpu().numpy(), ti.text(want))
    twin = _packed(want)
    assert np.array_equal(_plane_bytes(aln), _plane_bytes(twin))
    twin.close()
    aln.close()


def test_a_malformed_tree_and_bad_offsets_are_refused_before_a_launch(hiplib):
    import torch
    from tracs_amd import device as dev
    from tracs_amd._lib import TracsError
    rng = np.random.default_rng(12)
    n, L = 9, 300
    masks = _masks(n, L, rng)
    aln = _packed(masks)
    before = _plane_bytes(aln)
    parent, child = fr.random_tree(n, rng)
    lists, keep = _lists(len(parent), L, "all", rng)
    off, pos, dropped = _device_lists(lists, keep)
    with pytest.raises((TracsError, RuntimeError), match="2n - 3 edges"):
        dev.mask_subtrees(aln, parent[:-1], child[:-1], off[:-1], pos, dropped)
    swapped = child.copy()
    swapped[0], swapped[1] = child[1], child[0]
    with pytest.raises((TracsError, RuntimeError), match="creation order"):
        dev.mask_subtrees(aln, parent, swapped, off, pos, dropped)
    bad = off.clone()
    bad[3] = bad[2] - 1
    with pytest.raises((TracsError, RuntimeError), match="offsets decrease at edge 2"):
        dev.mask_subtrees(aln, parent, child, bad, pos, dropped)
    with pytest.raises((TracsError, RuntimeError), match="beyond the"):
        dev.mask_subtrees(aln, parent, child, off, pos[:-1], dropped[:-1])
    bad = off.clone()
    bad[0] = 1
    with pytest.raises((TracsError, RuntimeError), match=r"edge_off\[0\] must be 0"):
        dev.mask_subtrees(aln, parent, child, bad, pos, dropped)
    assert np.array_equal(_plane_bytes(aln), before)                                 # nothing was stored
    # an entry beyond L stores nothing (and is not counted)
    far = pos.clone()
    far[:] = L + 5
    assert dev.mask_subtrees(aln, parent, child, off, far, dropped) == 0
    assert np.array_equal(_plane_bytes(aln), before)
    one = _packed(masks[:1])
    e = np.zeros(0, np.uint32)
    assert dev.mask_subtrees(one, e, e, torch.zeros(1, dtype=torch.int64, device="cuda"), pos[:0], dropped[:0]) == 0
    one.close()
    aln.close()


def _brute(masks):
    m = np.asarray(masks, np.int64)
    n = m.shape[0]
    d, nn = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    for i in range(n):
        d[i] = ((m[i][None, :] & m) == 0).sum(axis=1)
        nn[i] = ((m[i][None, :] != 15) & (m != 15)).sum(axis=1)
    return d, nn


@pytest.mark.parametrize("kind", ["conserved", "partial codes"])
def test_the_per_pack_caches_are_rebuilt_after_a_mask(hiplib, kind):
    """one clone: the dense pair call, the mask, the dense pair call again; d and the compared sites are the brute force on the text the
    handle holds, both times -- site classes, lists, row slots and the encoding decided for the first pack would show here"""
    import torch
    from tracs_amd import device as dev
    rng = np.random.default_rng(99)
    n, L = 130, 6000
    base = rng.integers(0, 4, L)
    lineage = np.where(rng.random((3, L)) < 0.01, rng.integers(0, 4, (3, L)), base)
    seqs = np.where(rng.random((n, L)) < 0.001, rng.integers(0, 4, (n, L)), lineage[rng.integers(0, 3, n)])
    masks = (1 << seqs).astype(np.int64)
    masks = np.where(rng.random((n, L)) < 0.003, 15, masks)
    if kind == "partial codes":
        masks = np.where(rng.random((n, L)) < 0.002, rng.integers(1, 16, (n, L)), masks)
    src = _packed(masks)
    aln = dev.clone_alignment(src)

    def dense():
        d = torch.zeros((n, n), dtype=torch.int32, device="cuda")
        nn = torch.zeros((n, n), dtype=torch.int32, device="cuda")
        dev.pairsnp_dense(aln, d, nn)
        return np.triu(d.cpu().numpy(), 1), np.triu(nn.cpu().numpy(), 1)
    wd, wn = _brute(masks)
    d, nn = dense()
    assert np.array_equal(d, np.triu(wd, 1)) and np.array_equal(nn, np.triu(wn, 1))
    parent, child = fr.random_tree(n, rng)
    lists = [np.sort(rng.choice(L, 40, replace=False)).astype(np.int64) for _ in parent]
    keep = [rng.random(40) < 0.5 for _ in parent]
    want, cells, _ = ti.mask(masks, parent, child, lists, keep)
    assert dev.mask_subtrees(aln, parent, child, *_device_lists(lists, keep)) == cells > 1000
    wd, wn = _brute(want)
    assert not np.array_equal(np.triu(wd, 1), d)                                     # (the mask moved the distances)
    d, nn = dense()
    assert np.array_equal(d, np.triu(wd, 1)) and np.array_equal(nn, np.triu(wn, 1))
    assert np.array_equal(aln.unpack().cpu().numpy(), ti.text(want))
    aln.close()
    src.close()
