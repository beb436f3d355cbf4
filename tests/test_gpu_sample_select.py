"""The sample and pair rules on the GPU (csrc/sample_select.hip): the N counts per sample against numpy, the gathered planes byte for
byte against a pack of seqs[mask], the results on the gathered handle against the oracle on seqs[mask], the veto pass on a dense
panel, the errors."""
import ctypes as C

import numpy as np
import pytest

from sample_rules_common import G, check_plan, expected, files_keep, planted_input
from site_rules_common import is_n_table

pytestmark = pytest.mark.gpu


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


def _input(n, L, isn, partial=True):
    """planted input where there is room for it, a denser synthetic alignment for the small shapes"""
    from tracs_amd import synth
    if L >= 5000 and n >= 70:
        seqs, keep, plan = planted_input(n, L, isn)
        check_plan(seqs, isn, keep, plan)
    else:
        seqs = synth.alignment(n, L, seed=n + L, mu_lineage=3e-2, mu_sample=1e-2, p_n=0.08, p_partial=0.03, p_lower=0.05, p_other=0.03)
        keep = np.ones(L, bool)
        keep[L // 3:L // 3 + L // 4] = False
        keep[0] = keep[L - 1] = False
    if not partial:
        part = ~np.isin(seqs, np.frombuffer(b"ACGTN", np.uint8))
        seqs[part] = ord("A")
    return seqs, keep


@pytest.mark.parametrize("n,L", [(33, 129), (64, 5000), (65, 5000), (131, 30001)])
def test_sample_n_counts(hiplib, n, L):
    isn = is_n_table(hiplib)
    seqs, keep = _input(n, L, isn)
    seqs[1, :] = ord("N")                                  # a record that is N everywhere, one that never is, '-', a byte that is
    seqs[2, :] = ord("A")                                  # no letter, and a partial code
    seqs[4, ::3] = ord("-")
    seqs[4, 1::3] = 0x07
    seqs[4, 2::3] = ord("R")
    assert isn[ord("-")] and isn[0x07] and not isn[ord("R")]
    aln = _packed(seqs)
    is_n = isn[seqs]
    got = aln.sample_n_counts().cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (n,)
    assert np.array_equal(got, is_n.sum(axis=1))
    assert got[1] == L and got[2] == 0 and got[4] == L - len(range(2, L, 3))
    masked = aln.sample_n_counts(keep=keep).cpu().numpy()
    assert np.array_equal(masked, is_n[:, keep].sum(axis=1))
    assert masked[1] == keep.sum() and (masked != got).any()
    assert np.array_equal(aln.sample_n_counts(keep=np.ones(L, bool)).cpu().numpy(), got)
    one = np.zeros(L, bool); one[L - 1] = True             # the last column alone: the tail word of the last group
    assert np.array_equal(aln.sample_n_counts(keep=one).cpu().numpy(), is_n[:, L - 1].astype(np.int32))
    aln.close()


def _masks(n, seqs, isn, keep, rng):
    """name -> bool[n]"""
    m = {
        "everything": np.ones(n, bool),
        "first and last dropped": np.r_[False, np.ones(n - 2, bool), False],
        "half": rng.random(n) < 0.5,
        "one sample": np.arange(n) == n // 2,
        "last sample": np.arange(n) == n - 1,
    }
    m["half"][n // 2] = True
    if n > 64:
        few = np.zeros(n, bool); few[rng.choice(n, 60, replace=False)] = True          # n_pad shrinks: 131 -> 60 samples, 192 -> 64 slots
        m["fewer than 64 of more than 64"] = few
        sixty_four = np.zeros(n, bool); sixty_four[rng.choice(n, 64, replace=False)] = True
        m["exactly 64"] = sixty_four
    if seqs.shape[1] >= 5000 and n >= 70:
        m["sample rule"] = expected(seqs, isn, keep, G, None)["kept_samples"]
    return m


@pytest.mark.parametrize("partial", [False, True], ids=["acgtn", "partial codes"])
@pytest.mark.parametrize("n,L", [(33, 129), (70, 5000), (131, 30001)])
def test_selected_planes_byte_for_byte(hiplib, n, L, partial):
    isn = is_n_table(hiplib)
    seqs, keep = _input(n, L, isn, partial)
    src = _packed(seqs)
    before = _plane_bytes(src)
    rng = np.random.default_rng(n * L)
    shrunk = False
    for name, mask in _masks(n, seqs, isn, keep, rng).items():
        new = src.select_samples(mask)
        assert new.n == int(mask.sum()) and new.L == L, name
        twin = _packed(seqs[mask])
        a, b = _plane_bytes(new), _plane_bytes(twin)
        assert a.shape == b.shape and new.nbytes == twin.nbytes, name
        assert np.array_equal(a, b), (name, int((a != b).sum()))                         # pad samples, tail bits, pad groups and slack included
        shrunk |= new.nbytes < src.nbytes and (new.n + 63) // 64 < (n + 63) // 64
        if name != "everything":
            assert a.shape != before.shape or not np.array_equal(a, before), name
        new.close()
        twin.close()
    assert shrunk == (n > 64)
    assert np.array_equal(_plane_bytes(src), before)                                      # the source is left as it was
    src.close()


def _dense(aln, **kw):
    import torch
    from tracs_amd import device as dev
    n = aln.n
    d = torch.full((n, n), -1, dtype=torch.int32, device="cuda")
    nn = torch.full((n, n), -1, dtype=torch.int32, device="cuda")
    dev.pairsnp_dense(aln, d, nn, **kw)
    torch.cuda.synchronize()
    return d, nn


@pytest.mark.parametrize("n,L", [(70, 5000), (131, 30001)])
def test_results_on_the_selected_handle(hiplib, oracle, n, L):
    isn = is_n_table(hiplib)
    seqs, keep, plan = planted_input(n, L, isn)
    e = check_plan(seqs, isn, keep, plan)
    mask = e["kept_samples"]
    src = _packed(seqs)
    counts = src.sample_n_counts(keep=keep).cpu().numpy()
    assert np.array_equal(counts, e["n_counts"])
    assert np.array_equal(counts <= e["threshold"], mask)                                 # the rule from the device's own counts
    new = src.select_samples(mask)
    m = new.n
    er, ec, ed, enn = oracle.pairsnp_arrays(seqs[mask])
    iu = np.triu_indices(m, 1)
    assert np.array_equal(er.astype(np.int64), iu[0]) and np.array_equal(ec.astype(np.int64), iu[1])
    d, nn = _dense(new)
    assert np.array_equal(d.cpu().numpy().view(np.uint32)[iu], ed) and np.array_equal(nn.cpu().numpy().view(np.uint32)[iu], enn)
    # ... and the source still gives the result over every record
    ur, uc, ud, unn = oracle.pairsnp_arrays(seqs)
    d, nn = _dense(src)
    iu = np.triu_indices(n, 1)
    assert np.array_equal(d.cpu().numpy().view(np.uint32)[iu], ud) and np.array_equal(nn.cpu().numpy().view(np.uint32)[iu], unn)
    # the sample selection and the site selection commute: either order gives the planes of seqs[mask][:, cols]
    cols = files_keep(L)
    a, _ = new.select_sites(keep=cols)
    b0, _ = src.select_sites(keep=cols)
    b = b0.select_samples(mask)
    assert np.array_equal(_plane_bytes(a), _plane_bytes(b))
    for x in (a, b, b0, new, src):
        x.close()


@pytest.mark.parametrize("rows", ["all", "sub-range", "two files"])
def test_pairs_min_sites_on_a_panel(hiplib, rows):
    import torch
    from tracs_amd import device as dev
    isn = is_n_table(hiplib)
    n, L = 131, 5000
    seqs, keep, plan = planted_input(n, L, isn)            # (the dropped samples' N runs spread the compared-sites counts)
    aln = _packed(seqs)
    rb, re, cb = {"all": (0, n, 0), "sub-range": (n // 5, n // 2 + 3, 0), "two files": (0, 50, 50)}[rows]
    ld = n + 5                                             # columns behind n: never part of the cell set
    # every byte outside the cell set holds a cell the rule WOULD veto if the pass touched it: distance 0, compared over 0 sites
    d = torch.zeros((n, ld), dtype=torch.int32, device="cuda")
    nn = torch.zeros((n, ld), dtype=torch.int32, device="cuda")
    dev.pairsnp_dense(aln, d, nn, row_begin=rb, row_end=re, col_begin=cb)
    torch.cuda.synchronize()
    ii, jj = np.meshgrid(np.arange(n), np.arange(ld), indexing="ij")
    cell = (ii >= rb) & (ii < re) & (jj >= np.maximum(cb, ii + 1)) & (jj < n)
    exact_d = d.cpu().numpy().view(np.uint32).copy()
    T = int(np.median(exact_d[cell]))                      # a finite threshold: cells beyond it come back as the dense call leaves them
    d.zero_(); nn.zero_()
    dev.pairsnp_dense(aln, d, nn, row_begin=rb, row_end=re, col_begin=cb, dist_threshold=T)
    torch.cuda.synchronize()
    d0, n0 = d.cpu().numpy().view(np.uint32).copy(), nn.cpu().numpy().view(np.uint32).copy()
    inside = cell & (d0 <= T)
    assert inside.any() and (cell & (d0 > T)).any() and np.array_equal(d0[inside], exact_d[inside])
    M = int(np.sort(n0[inside])[inside.sum() // 2])        # a value that occurs, near the median: the >= boundary is hit
    veto = inside & (n0 < M)
    assert veto.any() and (inside & (n0 == M)).any() and (inside & (n0 > M)).any()
    dev.pairs_min_sites(d, nn, n, M, row_begin=rb, row_end=re, col_begin=cb, dist_threshold=T)
    torch.cuda.synchronize()
    d1, n1 = d.cpu().numpy().view(np.uint32), nn.cpu().numpy().view(np.uint32)
    want = d0.copy()
    want[veto] = 0xFFFFFFFF
    assert np.array_equal(d1, want)                        # vetoed cells; cells past the threshold, cells outside the set: as they were
    assert np.array_equal(n1, n0)
    assert (d1[~cell] == 0).all() and (n1[~cell] == 0).all()
    # the consumers' rule "unsigned cell <= threshold" now yields the eligible pairs only
    r, c, dd, cn = dev.coo_from_dense(d, nn, n, dist_threshold=T, row_begin=rb, row_end=re, col_begin=cb)
    ok = inside & ~veto
    assert np.array_equal(r.cpu().numpy(), ii[ok]) and np.array_equal(c.cpu().numpy(), jj[ok])
    assert np.array_equal(dd.cpu().numpy().view(np.uint32), d0[ok]) and (cn.cpu().numpy().view(np.uint32) >= M).all()
    # min_sites = 1 and a threshold of -1 change nothing
    dev.pairs_min_sites(d, nn, n, 1, row_begin=rb, row_end=re, col_begin=cb, dist_threshold=T)
    dev.pairs_min_sites(d, nn, n, 0xFFFFFFFF, row_begin=rb, row_end=re, col_begin=cb, dist_threshold=-1)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint32), want)
    aln.close()


def test_errors(hiplib):
    from tracs_amd import synth
    seqs = synth.alignment(20, 700, seed=2, p_n=0.05)
    src = _packed(seqs)
    with pytest.raises(ValueError) as e:
        src.select_samples(np.ones(19, bool))
    assert "19" in str(e.value) and "20" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        src.select_samples(np.zeros(20, bool))
    assert str(e.value) == "no sample left after the sample rule"
    with pytest.raises(RuntimeError) as e:
        src.sample_n_counts(keep=np.ones(699, bool))
    assert "699" in str(e.value) and "700" in str(e.value)
    h = C.c_void_p(7)
    assert hiplib.tracs_alignment_select_samples(src._h, None, C.byref(h), None) == -1 and not h.value
    assert hiplib.tracs_last_error() == b"tracs_alignment_select_samples: NULL argument"
    assert hiplib.tracs_alignment_select_samples(src._h, (C.c_uint8 * 20)(), None, None) == -1
    assert hiplib.tracs_alignment_sample_n_counts(src._h, None, 0, None, None) == -1
    assert hiplib.tracs_last_error() == b"tracs_alignment_sample_n_counts: NULL argument"
    assert hiplib.tracs_pairs_min_sites(None, None, 20, 20, 0, 20, 0, 5, 3, None) == -1
    one = src.select_samples(np.arange(20) == 4)           # one survivor is allowed: no pair
    assert one.n == 1
    one.close()
    src.close()
