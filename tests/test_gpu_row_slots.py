"""The rows' N sites as slots of 16-bit entries (csrc/site_lists.hip: row_slots_kernel, nn_rows_kernel<.., SLOTS>) instead of bitmaps:
the slot's line and load boundaries, the cap and the overflow fall-back to the stored N plane, the choice per call, row panels, row
splits and column chunks.  Pair results bit for bit against the oracle on all pairs (column chunks: slots against bitmaps).

A child process per case: TRACS_ROW_LISTS and TRACS_NN_LIST_K are read once per process.  TRACS_NN_LIST_K=1 makes every site
outside the dense class with two or more N samples a site whose N co-occurrences come from lists, at any n."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
BATCH = 8192                                                   # sites of a slot: 64 groups of 128
# entries of pair r's slot in batch 0: 63 | 64 a slot grows from one 128-byte line to two, 127 | 128 the walk needs its second load,
# 255 | 256 the cap and the first overflowed slot
BOUNDARY_COUNTS = [0, 1, 63, 64, 127, 128, 191, 192, 255, 256]


def _child(case, env, out=None):
    e = dict(os.environ)
    for k in ("TRACS_ROW_LISTS", "TRACS_NN_LIST_K", "TRACS_NN_LISTS", "TRACS_LIST_CAP"):
        e.pop(k, None)
    e["TRACS_NN_LIST_K"] = "1"
    e.update(env)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import scratch_poison; scratch_poison.enter_child(%r); import test_gpu_row_slots as T; T.run_case(%r, %r)" % (
        ROOT, os.path.join(ROOT, "tests"), "row_slots:%s:TRACS_ROW_LISTS=%s" % (case, e.get("TRACS_ROW_LISTS")), case, out)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=900, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    return res.stdout


def _consensus(n, L, rng, mu):
    seqs = np.tile(BASES[rng.integers(0, 4, size=L)], (n, 1))
    if mu:
        k = rng.poisson(mu * n * L)
        seqs[rng.integers(0, n, size=k), rng.integers(0, L, size=k)] = BASES[rng.integers(0, 4, size=k)]
    return seqs


def _iid_n(seqs, rows, p_n, rng):
    """N at p_n of the cells of `rows` (positions drawn with replacement: a few land twice)"""
    L = seqs.shape[1]
    k = rng.poisson(p_n * len(rows) * L)
    seqs[np.asarray(rows)[rng.integers(0, len(rows), size=k)], rng.integers(0, L, size=k)] = ord("N")


def _boundaries():
    """n = 64, three batches (the last ragged, 500 sites): samples 2 r and 2 r + 1 are both N at exactly c_r sites of batch 0 --
    nobody else is, so each such site has two N samples and a list --, and at other numbers of sites in batches 1 and 2"""
    n, L = 64, 2 * BATCH + 500
    rng = np.random.default_rng(11)
    seqs = _consensus(n, L, rng, 0.0)
    planted = np.zeros((n, L), dtype=bool)
    per_batch = [BOUNDARY_COUNTS, [3 * r + 2 for r in range(10)], [40 - 4 * r for r in range(10)]]
    for b, counts in enumerate(per_batch):
        lo, hi = b * BATCH, min(L, (b + 1) * BATCH)
        assert sum(counts) <= hi - lo
        sites = lo + rng.permutation(hi - lo)[:sum(counts)]              # distinct sites, anywhere in the batch
        at = 0
        for r, c in enumerate(counts):
            planted[2 * r, sites[at:at + c]] = planted[2 * r + 1, sites[at:at + c]] = True
            at += c
    free = np.nonzero(~planted.any(axis=0))[0]                           # a few mutations, away from the planted sites
    k = 300
    seqs[rng.integers(20, n, size=k), free[rng.integers(0, free.size, size=k)]] = BASES[rng.integers(0, 4, size=k)]
    seqs[planted] = ord("N")
    return seqs, planted


def _extremes(n, p_n):
    """one sample N at every site (every slot of its row overflows), one without any N (every count 0), the others p_n iid"""
    L = 2 * BATCH + 500
    rng = np.random.default_rng(12)
    seqs = _consensus(n, L, rng, 3e-4)
    _iid_n(seqs, [s for s in range(n) if s not in (5, 9)], p_n, rng)
    seqs[5, :] = ord("N")
    seqs[9, :] = _consensus(1, L, np.random.default_rng(12), 0.0)[0]     # (the consensus itself: no N, no mutation)
    return seqs


def _iid(n, L, p_n, seed=13, mu=3e-4):
    rng = np.random.default_rng(seed)
    seqs = _consensus(n, L, rng, mu)
    _iid_n(seqs, list(range(n)), p_n, rng)
    return seqs


def _few_heavy_rows():
    """5 of 300 samples carry 25 % N, the others none: rows of ~17 000 listed N sites, cut over several workgroups (grid.z), ~1 400
    per slot -- every slot of theirs overflowed, all others empty; 23 entries per slot on average, so the rule chooses slots"""
    n, L = 300, 100000
    rng = np.random.default_rng(14)
    seqs = _consensus(n, L, rng, 1e-4)
    for s in (3, 77, 150, 151, 299):
        seqs[s, rng.random(L) < 0.25] = ord("N")
    return seqs


def _run(seqs, row_lists, bitmap_sites=None, panels=None):
    """whole-matrix d and nn against the oracle, the row source in use, the expanded bitmap (tracs_debug_lists what = 8) against numpy"""
    import torch
    from oracle import oracle as O
    from tracs_amd import _lib, device as dev
    lib = _lib.load()
    n, L = seqs.shape
    er, ec, ed, enn = O.pairsnp_arrays(seqs, n_threads=8)
    ri, ci = er.astype(np.int64), ec.astype(np.int64)
    aln = dev.Alignment(n, L)
    aln.pack(seqs)
    d = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    nn = torch.zeros_like(d)
    try:
        lib.tracs_debug_force_site_classes(1)
        dev.pairsnp_dense(aln, d, nn)
        assert aln.site_classes is not None
        ls = aln.list_stats
        print("list_stats", ls, flush=True)
        dh, nh = d.cpu().numpy(), nn.cpu().numpy()
        assert np.array_equal(dh[ri, ci], ed.astype(np.int32)), "d differs from the oracle"
        assert np.array_equal(nh[ri, ci], enn.astype(np.int32)), "nn differs from the oracle"
        if row_lists is not None:
            assert ls.get("bitmaps") is True, ls                        # a row source exists ...
            assert ls.get("row_lists") is row_lists, ls                 # ... and it is the one expected
            assert (ls["row_list_lines"] > 0) == row_lists, ls
        if bitmap_sites is not None or (row_lists is not None and ls.get("bitmaps")):
            sizes = np.zeros(8, dtype=np.uint64)
            assert lib.tracs_debug_lists(aln._h, 0, sizes.ctypes.data_as(C.c_void_p), 64) == 64
            tgroups = int(sizes[3])
            T = np.empty(n * tgroups * 4, dtype=np.uint32)
            assert lib.tracs_debug_lists(aln._h, 8, T.ctypes.data_as(C.c_void_p), T.nbytes) == T.nbytes
            bits = np.unpackbits(T.view(np.uint8).reshape(n, -1), axis=1, bitorder="little")
            assert not bits[:, L:].any(), "bits behind the last site"
            bits = bits[:, :L].astype(bool)
            isN = seqs == ord("N")
            col = bits.any(axis=0)
            # per site either the N plane's column (a site whose N co-occurrences come from lists: two or more N samples) or nothing
            assert (bits[:, col] == isN[:, col]).all()
            assert (isN[:, col].sum(axis=0) >= 2).all()
            if bitmap_sites is not None:
                assert col[bitmap_sites].all(), "a planted site has no list"
        if panels:
            aln.hint_rows(panels)
            dp = torch.zeros_like(d)
            npn = torch.zeros_like(d)
            for r0, r1 in panels:
                dev.pairsnp_dense(aln, dp, npn, row_begin=r0, row_end=r1)
            assert aln.list_stats.get("row_lists") is row_lists
            assert np.array_equal(dp.cpu().numpy()[ri, ci], dh[ri, ci]) and np.array_equal(npn.cpu().numpy()[ri, ci], nh[ri, ci]), "panels differ from the whole matrix"
            aln.hint_rows([])
    finally:
        lib.tracs_debug_force_site_classes(-2)
    aln.close()
    return ls


def _column_chunks(out):
    """n = 37 000: two column chunks of the row in LDS (nn_rows_kernel<CLAMP = true>); one panel of 64 rows, saved for the parent"""
    import torch
    from tracs_amd import _lib, device as dev
    lib = _lib.load()
    n, L, rows = 37000, 2048, 64
    seqs = _iid(n, L, 0.005, seed=15, mu=1e-4)
    aln = dev.Alignment(n, L)
    aln.pack(seqs)
    d = torch.zeros((rows, n), dtype=torch.int32, device="cuda")
    nn = torch.zeros_like(d)
    try:
        lib.tracs_debug_force_site_classes(1)
        dev.pairsnp_dense(aln, d, nn, row_begin=0, row_end=rows)
        ls = aln.list_stats
    finally:
        lib.tracs_debug_force_site_classes(-2)
    print("list_stats", ls, flush=True)
    assert ls.get("bitmaps") is True and ls.get("row_lists") is (os.environ["TRACS_ROW_LISTS"] == "1"), ls
    assert tuple(nn.shape) == (rows, n)
    np.save(out, np.stack([d.cpu().numpy(), nn.cpu().numpy()]))
    aln.close()


def run_case(case, out=None):
    if case == "boundaries":
        seqs, planted = _boundaries()
        both = planted[0::2] & planted[1::2]
        assert [int(x) for x in both[:10, :BATCH].sum(axis=1)] == BOUNDARY_COUNTS
        _run(seqs, True, bitmap_sites=np.nonzero(planted.any(axis=0))[0])
    elif case == "extremes_n64":
        # (at 64 samples nearly half of the sites would carry a list next to the all-N sample: beyond the lists' share of the planes'
        # size, so the classes may come without these lists -- the results must be the oracle's either way)
        _run(_extremes(64, 0.01), None)
    elif case == "extremes_n256":
        _run(_extremes(256, 0.003), True)
    elif case == "iid_1pct":
        forced = os.environ.get("TRACS_ROW_LISTS")
        _run(_iid(700, 20000, 0.01), True if forced is None else forced == "1")
    elif case == "iid_3pct":
        _run(_iid(700, 20000, 0.03), False)
    elif case == "panels":
        _run(_iid(700, 20000, 0.01), True, panels=[(0, 250), (250, 700)])
    elif case == "few_heavy_rows":
        ls = _run(_few_heavy_rows(), True)
        assert ls["row_splits"] >= 2, ls
    elif case == "column_chunks":
        _column_chunks(out)
    else:
        raise ValueError(case)
    print("ok", case, flush=True)


def test_slot_and_line_boundaries(hiplib):
    """counts 0, 1, 63 | 64, 127 | 128, 191 | 192, 255 | 256 in batch 0 and other counts in batches 1 and 2 of the same samples"""
    _child("boundaries", {})


@pytest.mark.parametrize("case", ["extremes_n64", "extremes_n256"])
def test_extremes(hiplib, case):
    """a sample that is N everywhere (every slot overflowed: read from the stored N plane) and one without any N (every count 0)
    among iid samples -- at n = 64, and, because the lists of that alignment may be refused as too large beside 64 samples' planes,
    at n = 256 with 0.3 % N, where they are not and the slots must be in use"""
    _child(case, {})


@pytest.mark.parametrize("forced", ["1", "0", None], ids=["slots", "bitmaps", "rule"])
def test_both_sources_agree(hiplib, forced):
    """n = 700, L = 20 000, 1 % N: d and nn are the oracle's with slots, with bitmaps and with the library's own choice -- which is
    slots (82 entries per slot on average)"""
    _child("iid_1pct", {} if forced is None else {"TRACS_ROW_LISTS": forced})


def test_rule_chooses_bitmaps_at_3_percent(hiplib):
    """the same alignment with 3 % N: 246 entries per slot on average, beyond the rule's 160 -- bitmaps"""
    _child("iid_3pct", {})


def test_row_panels(hiplib):
    """two uneven row panels after hint_rows give the whole-matrix call's cells"""
    _child("panels", {})


def test_row_splits_of_overflowed_rows(hiplib):
    """5 of 300 samples with 25 % N: long rows cut over several workgroups, every slot of theirs overflowed"""
    _child("few_heavy_rows", {})


def test_column_chunks(hiplib, tmp_path):
    """n = 37 000 (two column chunks, CLAMP = true), L = 2 048, 0.5 % N, a panel of 64 rows: nn from slots equals nn from bitmaps
    (source against source: the bitmap walk's own correctness at this size is scripts/check_large_n.py's business)"""
    outs = []
    for forced in ("1", "0"):
        outs.append(str(tmp_path / ("panel_%s.npy" % forced)))
        _child("column_chunks", {"TRACS_ROW_LISTS": forced}, outs[-1])
    a, b = np.load(outs[0]), np.load(outs[1])
    assert a.shape == (2, 64, 37000)
    assert np.array_equal(a[1], b[1]), "nn differs between slots and bitmaps"
    assert np.array_equal(a[0], b[0]), "d differs between slots and bitmaps"
    assert a[1].any()
