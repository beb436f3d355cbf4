"""The per-site census (csrc/msa_out.hip: site_census_kernel): the six counts against numpy, the differs bitmap against its definition
-- two samples with disjoint allele masks --, that definition against brute-force SNP distances, and a handle that went through
select_samples and select_sites (pad samples and stale columns must not count)."""
import numpy as np
import pytest

from site_rules_common import standard_input

pytestmark = pytest.mark.gpu

# the census kernel's constants: 64 lanes over samples, 8-bit sliced counters -> a lane's counters are flushed every 255 samples
LANES, CHUNK = 64, 255
N_TWO_FLUSHES = 2 * LANES * CHUNK + 360                     # 33 000: two full chunks and a third, short one
SHAPES = [(33, 129), (70, 5000), (131, 30001), (2500, 300), (N_TWO_FLUSHES, 129)]
DIFFERING_UNPLANTED = {(33, 129): 87, (70, 5000): 961, (131, 30001): 9902}
PLANT0 = 20


def _mask_table(hiplib):
    return np.array([hiplib.tracs_debug_iupac_mask(ch) for ch in range(256)], np.uint8)


def _census_numpy(masks):
    """masks uint8 [n, L] -> (counts int64 [6, L], differs bool [L]) from the definitions"""
    counts = np.stack([(masks == m).sum(axis=0) for m in (1, 2, 4, 8, 15)] + [np.isin(masks, (3, 5, 6, 7, 9, 10, 11, 12, 13, 14)).sum(axis=0)])
    present = [None] + [(masks == m).any(axis=0) for m in range(1, 15)]
    differs = np.zeros(masks.shape[1], bool)
    for a in range(1, 15):
        for b in range(a + 1, 15):
            if a & b == 0:
                differs |= present[a] & present[b]
    return counts, differs


def _unplanted(n, L):
    from tracs_amd import synth
    if (n, L) == (33, 129):                                 # the small case of test_selected_planes_byte_for_byte with partial codes
        return synth.alignment(n, L, 3, mu_lineage=3e-2, mu_sample=1e-2, p_n=0.05, p_partial=0.05, p_other=0.02)
    if L >= 5000:
        return standard_input(n, L)[0]
    return synth.alignment(n, L, seed=n + L, mu_lineage=3e-3, mu_sample=1e-3, p_n=0.05, p_partial=0.02, p_lower=0.05, p_other=0.03)


def _plant(seqs):
    """the edge columns -> {name: (column, differs)}"""
    n, L = seqs.shape
    half = np.arange(n) % 2 == 0
    plan = {}

    def two(name, col, x, y, differs):
        seqs[half, col] = ord(x)
        seqs[~half, col] = ord(y)
        plan[name] = (col, differs)
    two("all A", PLANT0, "A", "A", False)
    two("all N", PLANT0 + 1, "N", "N", False)
    two("A and N", PLANT0 + 2, "A", "N", False)
    two("R and A", PLANT0 + 3, "R", "A", False)           # overlap
    two("R and C", PLANT0 + 4, "R", "C", True)            # one one-hot letter present
    two("R and Y", PLANT0 + 5, "R", "Y", True)            # none
    two("M and K", PLANT0 + 6, "M", "K", True)
    two("V and T", PLANT0 + 7, "V", "T", True)
    two("- and A", PLANT0 + 8, "-", "A", False)
    seqs[:, PLANT0 + 9] = ord("A")
    seqs[n // 2, PLANT0 + 9] = ord("G")
    plan["one G among A"] = (PLANT0 + 9, True)
    seqs[:, L - 1] = ord("c")                               # the last valid site of the last group (L = 129: its only one),
    seqs[n - 1, L - 1] = ord("T")                           # decided by the last sample alone
    plan["last site"] = (L - 1, True)
    return plan


@pytest.fixture(scope="module", params=SHAPES, ids=["%dx%d" % s for s in SHAPES])
def case(request, hiplib):
    n, L = request.param
    table = _mask_table(hiplib)
    seqs = _unplanted(n, L)
    if (n, L) in DIFFERING_UNPLANTED:
        assert int(_census_numpy(table[seqs])[1].sum()) == DIFFERING_UNPLANTED[(n, L)]
    plan = _plant(seqs)
    masks = table[seqs]
    counts, differs = _census_numpy(masks)
    # the input can tell a wrong census from a right one
    assert 0 < differs.sum() < L and set(np.unique(masks).tolist()) == set(range(1, 16))
    return dict(n=n, L=L, seqs=seqs, masks=masks, counts=counts, differs=differs, plan=plan)


def _packed(seqs):
    from tracs_amd import device as dev
    a = dev.Alignment(*seqs.shape)
    a.pack(np.ascontiguousarray(seqs))
    return a


def test_counts_and_differs(case):
    import torch
    n, L = case["n"], case["L"]
    aln = _packed(case["seqs"])
    counts, differs = aln.site_census()
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (6, L) and counts.is_cuda
    assert differs.dtype == bool and differs.shape == (L,)
    got = counts.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, case["counts"]), np.argwhere(got != case["counts"])[:5]
    assert (got.sum(axis=0) == n).all()
    assert np.array_equal(differs, case["differs"]), np.flatnonzero(differs != case["differs"])[:10]
    for name, (col, want) in case["plan"].items():
        assert bool(differs[col]) == want, name
    col = case["plan"]["all N"][0]
    assert got[4, col] == n and got[:4, col].sum() == 0
    col = case["plan"]["R and A"][0]
    assert got[5, col] == (n + 1) // 2 and got[0, col] == n // 2
    col = case["plan"]["- and A"][0]
    assert got[4, col] == (n + 1) // 2
    # again on the same handle: the same answer (nothing is left behind between calls), and counts alone / differs alone
    counts2, differs2 = aln.site_census()
    assert torch.equal(counts, counts2) and np.array_equal(differs, differs2)
    aln.close()


def test_c_entry_point_optional_outputs(hiplib):
    import ctypes as C

    import torch
    n, L = 33, 129
    table = _mask_table(hiplib)
    seqs = _unplanted(n, L)
    _plant(seqs)
    want_counts, want_differs = _census_numpy(table[seqs])
    aln = _packed(seqs)
    words = np.zeros((L + 63) // 64, np.uint64)
    nd = C.c_size_t(0)
    u64p = C.POINTER(C.c_uint64)
    assert hiplib.tracs_alignment_site_census(aln._h, None, words.ctypes.data_as(u64p), C.byref(nd), None) == 0
    assert nd.value == want_differs.sum()
    from tracs_amd.sites import bitmap_to_bool
    assert np.array_equal(bitmap_to_bool(words, L), want_differs)
    assert int(words[-1]) >> ((L - 1) % 64 + 1) == 0                                       # no bit at or beyond L
    nd2 = C.c_size_t(0)
    assert hiplib.tracs_alignment_site_census(aln._h, None, None, C.byref(nd2), None) == 0 and nd2.value == nd.value
    counts = torch.full((6, L), -1, dtype=torch.int32, device="cuda")
    assert hiplib.tracs_alignment_site_census(aln._h, C.c_void_p(counts.data_ptr()), None, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert hiplib.tracs_alignment_site_census(None, None, None, None, None) == -1
    aln.close()


def test_differs_is_what_changes_a_distance(hiplib):
    """brute force on (33, 129): d(i, j) = the sites with disjoint masks.  Deleting every non-differing column changes no distance;
    deleting any one differing column lowers some pair's."""
    table = _mask_table(hiplib)
    seqs = _unplanted(33, 129)
    _plant(seqs)
    masks = table[seqs]
    aln = _packed(seqs)
    _, differs = aln.site_census()
    aln.close()

    def dist(m):
        return ((m[:, None, :] & m[None, :, :]) == 0).sum(axis=2)
    full = dist(masks)
    assert full.max() > 0 and np.array_equal(dist(masks[:, differs]), full)
    assert 0 < differs.sum() < 129
    for col in np.flatnonzero(differs):
        keep = np.ones(129, bool)
        keep[col] = False
        assert (dist(masks[:, keep]) < full).any(), col
    for col in np.flatnonzero(~differs):
        keep = np.ones(129, bool)
        keep[col] = False
        assert np.array_equal(dist(masks[:, keep]), full), col


def test_after_select_samples_and_select_sites(hiplib):
    """131 -> 60 samples (n_pad shrinks from 192 to 64), then a column selection: the census of the result is numpy's on the cut
    arrays -- the samples that left and the columns that left must not count"""
    table = _mask_table(hiplib)
    n, L = 131, 30001
    seqs = _unplanted(n, L)
    _plant(seqs)
    rng = np.random.default_rng(5)
    keep_s = np.zeros(n, bool)
    keep_s[rng.choice(n, 60, replace=False)] = True
    keep_c = rng.random(L) < 0.6
    keep_c[PLANT0:PLANT0 + 10] = True
    src = _packed(seqs)
    fewer = src.select_samples(keep_s)
    cut, kept = fewer.select_sites(keep=keep_c)
    assert cut.n == 60 and cut.L == keep_c.sum() and np.array_equal(kept, keep_c)
    want_counts, want_differs = _census_numpy(table[seqs[keep_s][:, keep_c]])
    full_counts, full_differs = _census_numpy(table[seqs][:, keep_c])
    assert not np.array_equal(want_differs, full_differs) and 0 < want_differs.sum() < cut.L       # the samples that left matter
    counts, differs = cut.site_census()
    got = counts.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, want_counts) and (got.sum(axis=0) == 60).all()
    assert np.array_equal(differs, want_differs)
    # and the sample selection alone, on all columns
    want_counts, want_differs = _census_numpy(table[seqs[keep_s]])
    counts, differs = fewer.site_census()
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), want_counts) and np.array_equal(differs, want_differs)
    for a in (cut, fewer, src):
        a.close()
