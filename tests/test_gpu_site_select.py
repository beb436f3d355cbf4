"""Site rules on the GPU (csrc/site_select.hip): the N counts per site, the selected planes byte for byte against a pack of the
column-deleted sequences, the results on the selected handle against the oracle on seqs[:, kept], the returned bitmap, the errors."""
import ctypes as C
import math

import numpy as np
import pytest

from site_rules_common import is_n_table, standard_input, standard_rule

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


@pytest.mark.parametrize("n,L", [(33, 129), (70, 5000), (700, 9000), (2500, 300)])
def test_site_n_counts(hiplib, n, L):
    from tracs_amd import synth
    isn = is_n_table(hiplib)
    seqs = synth.alignment(n, L, seed=n + L, mu_lineage=3e-3, mu_sample=1e-3, p_n=0.05, p_partial=0.02, p_lower=0.05, p_other=0.03)
    seqs[:, L // 2] = ord("N")                              # a column where every sample is N, one where nobody is, '-' and a byte
    seqs[:, L // 3] = ord("A")                              # that is no letter at all
    seqs[::3, 5] = ord("-")
    seqs[1::3, 5] = 0x07
    seqs[2::3, 5] = ord("R")
    assert isn[ord("-")] and isn[0x07] and not isn[ord("R")] and not isn[ord("r")] and isn[ord("n")]
    aln = _packed(seqs)
    got = aln.site_n_counts().cpu().numpy()
    expect = isn[seqs].sum(axis=0)
    assert got.dtype == np.int32 and got.shape == (L,)
    assert np.array_equal(got, expect)
    assert got[L // 2] == n and got[L // 3] == 0 and got[5] == n - len(range(2, n, 3))
    aln.close()


def _selections(n, L, seqs, isn, rng):
    """name -> (keep bool[L] or None, max_n_samples or None)"""
    def dropped(*ranges):
        k = np.ones(L, bool)
        for s, e in ranges:
            k[s:min(e, L)] = False
        return k
    one_in_300 = np.zeros(L, bool); one_in_300[::300] = True
    one = np.zeros(L, bool); one[L * 2 // 3] = True
    mult = np.zeros(L, bool); mult[rng.choice(L, 128 * max(1, int(L * 0.7) // 128), replace=False)] = True
    sel = {
        "identity": (np.ones(L, bool), None),
        "first and last": (dropped((0, 1), (L - 1, L)), None),
        "whole groups": (dropped((128, 384)), None),
        "runs off the word boundary": (dropped((37, 91), (200, 333), (1000, 1001), (4097, 4999)), None),
        "half": (rng.random(L) < 0.5, None),
        "one percent dropped": (rng.random(L) >= 0.01, None),
        "one in 300": (one_in_300, None),
        "one column": (one, None),
        "multiple of 128": (mult, None),
        "N rule alone": (None, math.floor(0.03 * n)),
        "half and N rule": (rng.random(L) < 0.5, math.floor(0.03 * n)),
    }
    assert one_in_300.sum() < 128 and mult.sum() % 128 == 0
    if L >= 5000:
        keep, max_n, kept = standard_rule(seqs, isn)
        sel["standard rule"] = (keep, max_n)
    return sel


@pytest.mark.parametrize("partial", [False, True], ids=["acgtn", "partial codes"])
@pytest.mark.parametrize("n,L", [(33, 129), (70, 5000), (131, 30001)])
def test_selected_planes_byte_for_byte(hiplib, n, L, partial):
    isn = is_n_table(hiplib)
    if L >= 5000:
        seqs, _ = standard_input(n, L)
        if not partial:
            from tracs_amd import synth
            clean = synth.alignment(n, L, 11, mu_lineage=3e-3, mu_sample=1e-3, p_n=0.02, p_partial=0.0)
            part = ~np.isin(seqs, np.frombuffer(b"ACGTN", np.uint8))
            seqs[part] = clean[part]
    else:
        from tracs_amd import synth
        seqs = synth.alignment(n, L, 3, mu_lineage=3e-2, mu_sample=1e-2, p_n=0.05, p_partial=0.05 if partial else 0.0,
                               p_other=0.02 if partial else 0.0)
    src = _packed(seqs)
    before = _plane_bytes(src)
    n_count = isn[seqs].sum(axis=0)
    rng = np.random.default_rng(n * L)
    for name, (keep, max_n) in _selections(n, L, seqs, isn, rng).items():
        expect = np.ones(L, bool) if keep is None else keep.copy()
        if max_n is not None:
            expect &= n_count <= max_n
        assert expect.any(), name
        new, kept = src.select_sites(keep=keep, max_n_samples=max_n)
        assert kept.dtype == bool and np.array_equal(kept, expect), name                 # the returned bitmap and its population
        assert new.L == int(expect.sum()) and new.n == n, name
        twin = _packed(seqs[:, expect])
        a, b = _plane_bytes(new), _plane_bytes(twin)
        assert a.shape == b.shape and new.nbytes == twin.nbytes, name
        assert np.array_equal(a, b), (name, int((a != b).sum()))                         # pads and slack included
        new.close()
        twin.close()
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
    import torch
    from tracs_amd import device as dev
    isn = is_n_table(hiplib)
    seqs, _ = standard_input(n, L)
    keep, max_n, kept = standard_rule(seqs, isn)
    r, c, ed, enn = oracle.pairsnp_arrays(seqs[:, kept])
    ur, uc, ud, unn = oracle.pairsnp_arrays(seqs)
    ef, uf = oracle.filter_recomb_pairs(seqs[:, kept], r, c, 4), oracle.filter_recomb_pairs(seqs, ur, uc, 4)
    assert (ed != ud).any() and (enn != unn).any() and (ef != uf).any()                   # a no-op selection cannot pass
    src = _packed(seqs)
    new, got_kept = src.select_sites(keep=keep, max_n_samples=max_n)
    assert np.array_equal(got_kept, kept) and new.L == kept.sum()
    iu = np.triu_indices(n, 1)
    ri, ci = r.astype(np.int64), c.astype(np.int64)
    assert np.array_equal(ri, iu[0]) and np.array_equal(ci, iu[1])

    def check(aln, xd, xnn, xf):
        d, nn = _dense(aln)
        dh, nh = d.cpu().numpy().view(np.uint32), nn.cpu().numpy().view(np.uint32)
        assert np.array_equal(dh[iu], xd) and np.array_equal(nh[iu], xnn)
        # thresholded: exact within the threshold, beyond it (as unsigned) otherwise
        T = int(np.median(xd))
        dt, nt = _dense(aln, dist_threshold=T)
        dth, nth = dt.cpu().numpy().view(np.uint32)[iu], nt.cpu().numpy().view(np.uint32)[iu]
        inside = xd <= T
        assert inside.any() and (~inside).any()
        assert np.array_equal(dth[inside], xd[inside]) and np.array_equal(nth[inside], xnn[inside]) and (dth[~inside] > T).all()
        # a row panel against a column block
        rb, re, cb = n // 5, n // 2 + 3, n // 3
        dp, np_ = _dense(aln, row_begin=rb, row_end=re, col_begin=cb)
        cell = (ri >= rb) & (ri < re) & (ci >= cb)
        dph, nph = dp.cpu().numpy().view(np.uint32), np_.cpu().numpy().view(np.uint32)
        assert np.array_equal(dph[ri[cell], ci[cell]], xd[cell]) and np.array_equal(nph[ri[cell], ci[cell]], xnn[cell])
        written = np.zeros((n, n), bool); written[ri[cell], ci[cell]] = True
        assert (dp.cpu().numpy()[~written] == -1).all()
        # the recombination filter on every pair
        tr, tc = torch.from_numpy(ri.astype(np.int32)).cuda(), torch.from_numpy(ci.astype(np.int32)).cuda()
        td = torch.from_numpy(xd.astype(np.int32)).cuda()
        f = dev.filter_recomb_pairs(aln, tr, tc, td).cpu().numpy().view(np.uint32)
        assert np.array_equal(f, xf)

    check(new, ed, enn, ef)
    check(src, ud, unn, uf)                                                                # the source still gives the unmasked result
    new.close()
    src.close()


def test_errors(hiplib):
    from tracs_amd import synth
    seqs = synth.alignment(20, 700, seed=2, p_n=0.05)
    seqs[:, 10] = ord("N")
    src = _packed(seqs)
    with pytest.raises(RuntimeError) as e:
        src.select_sites(keep=np.ones(699, bool))
    assert "699" in str(e.value) and "700" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        src.select_sites(keep=np.zeros(700, bool))
    assert str(e.value) == "no site left after the site rules"
    only = np.zeros(700, bool); only[10] = True                    # the files leave one column, the N rule drops it
    with pytest.raises(RuntimeError) as e:
        src.select_sites(keep=only, max_n_samples=19)
    assert str(e.value) == "no site left after the site rules"
    h, nk = C.c_void_p(), C.c_size_t(7)
    words = np.zeros(11, np.uint64)
    rc = hiplib.tracs_alignment_select_sites(src._h, words.ctypes.data_as(C.POINTER(C.c_uint64)), 700, 0xFFFFFFFF, C.byref(h), None, C.byref(nk), None)
    assert rc == -1 and not h.value and nk.value == 0 and hiplib.tracs_last_error() == b"no site left after the site rules"
    new, kept = src.select_sites(keep=only, max_n_samples=20)      # ... and with the rule one sample wider it stays
    assert new.L == 1 and kept.sum() == 1
    new.close()
    src.close()


def test_fasta_entry_points(hiplib, oracle, tmp_path):
    """tracs_pairsnp_sites / tracs_nearest_sites / tracs_distance_open_sites: no rule = the plain entry points; a rule = the oracle on
    seqs[:, kept], the N rule counted over both files of a two-file run."""
    from tracs_amd import api, synth
    from tracs_amd.sites import Sites
    isn = is_n_table(hiplib)
    n, L = 70, 5000
    seqs, _ = standard_input(n, L)
    keep, max_n, kept = standard_rule(seqs, isn)
    fa, fb, fc = str(tmp_path / "a.fa"), str(tmp_path / "b.fa"), str(tmp_path / "c.fa")
    names = ["s%d" % i for i in range(n)]
    synth.write_fasta(fa, seqs, names=names, width=60)
    synth.write_fasta(fb, seqs[:25], names=names[:25])
    synth.write_fasta(fc, seqs[25:], names=names[25:])

    def same(x, y):
        assert len(x) == len(y) == 6
        for u, v in zip(x, y):
            assert (u == v) if isinstance(u, list) else np.array_equal(u, v)
    for files in ([fa], [fb, fc]):
        same(api.pairsnp_arrays(files, dist=40, filter=True), api.pairsnp_arrays(files, dist=40, filter=True, sites=Sites()))
        same(api.nearest_arrays(files, 3), api.nearest_arrays(files, 3, sites=Sites()))
    hn, hp = api.distance_histogram([fa]), api.distance_histogram([fa], sites=Sites())
    assert hn[0] == hp[0] and all(np.array_equal(hn[1]["snp"][k], hp[1]["snp"][k]) for k in hn[1]["snp"])

    info = {}
    r, c, d, nm, f, nn = api.pairsnp_arrays([fa], filter=True, sites=Sites(keep, max_n), info=info)
    er, ec, ed, enn = oracle.pairsnp_arrays(seqs[:, kept])
    assert info["seqlen"] == kept.sum() and nm == names
    assert np.array_equal(r, er) and np.array_equal(c, ec) and np.array_equal(d, ed) and np.array_equal(nn, enn)
    assert np.array_equal(f, oracle.filter_recomb_pairs(seqs[:, kept], er, ec, 4))
    ur, uc, ud, unn = oracle.pairsnp_arrays(seqs)
    assert (ed != ud).any()
    # two files: the same kept columns (the N rule counts all 70 samples), the cross pairs only
    r, c, d, nm, f, nn = api.pairsnp_arrays([fb, fc], sites=Sites(keep, max_n))
    er, ec, ed, enn = oracle.pairsnp_arrays(seqs[:, kept], n0=25)
    assert np.array_equal(r, er) and np.array_equal(c, ec) and np.array_equal(d, ed) and np.array_equal(nn, enn)
    # a rule on one file alone counts its own samples: floor(0.2 * 25) of 25
    sub_kept = keep & (isn[seqs[:25]].sum(axis=0) <= 5)
    r, c, d, nm, f, nn = api.pairsnp_arrays([fb], sites=Sites(keep, 5))
    er, ec, ed, enn = oracle.pairsnp_arrays(seqs[:25][:, sub_kept])
    assert np.array_equal(d, ed) and np.array_equal(nn, enn)
    # nearest under the rule: each sample's 3 nearest by (d, j) over the kept columns
    r, c, d, nm, f, nn = api.nearest_arrays([fa], 3, sites=Sites(keep, max_n))
    er, ec, ed, enn = oracle.pairsnp_arrays(seqs[:, kept])
    D = np.zeros((n, n), np.int64); D[er.astype(int), ec.astype(int)] = ed; D = D + D.T
    for s in range(n):
        order = sorted((int(D[s, j]), j) for j in range(n) if j != s)[:3]
        assert [int(x) for x in c[r == s]] == [j for _, j in order] and [int(x) for x in d[r == s]] == [x for x, _ in order]
    with pytest.raises(RuntimeError) as e:
        api.pairsnp_arrays([fa], sites=Sites(np.ones(L - 1, bool)))
    assert str(L - 1) in str(e.value) and str(L) in str(e.value)
    with pytest.raises(RuntimeError) as e:
        api.pairsnp_arrays([fa], sites=Sites(np.zeros(L, bool)))
    assert str(e.value) == "no site left after the site rules"
