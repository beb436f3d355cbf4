"""The SNP sites of listed pairs (csrc/pair_sites.hip) on the GPU: sites, both allele masks and the recombination
filter's verdict per SNP.

Brute force: n = 70 samples (n_pad = 128, sample indices beyond 64) with every IUPAC code, N, '-' and lower case, at lengths around
the word (32), the group (128) and a wave's sweep of 64 words (4133: a second sweep and a ragged tail); the masks are written here
from the IUPAC table and every list runs on both kernel forms (TRACS_PAIR_SITES_LANES_MIN).  Everything is an exact integer.
Verdicts: bit for bit against tests/golden/pair_sites_hp_golden.json (the definition at 50 digits) on the crafted pairs of
tests/test_gpu_filter_hp.py, and by count against the oracle's filtered distances on a random alignment with planted dense runs.
Rows: tracs_distance_pair_sites' CSV against the brute force, split into batches and refused above max_entries."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(HERE, "golden", "pair_sites_hp_golden.json")
LETTERS = "XACMGRSVTWYHKDBN"                       # the canonical letter of a mask: A = 1, C = 2, G = 4, T = 8
FORMS = {"wave": "1000000000", "lanes": "0"}       # TRACS_PAIR_SITES_LANES_MIN: a wave per pair / a pair per lane
LENGTHS = (1, 31, 32, 33, 127, 128, 129, 4133)
N = 70
_CACHE = {}


def _mask_table():
    """byte -> allele mask, from the IUPAC table: the letters in either case, everything else (N, '-', ..) is 15"""
    t = np.full(256, 15, np.uint8)
    for m, ch in enumerate(LETTERS):
        if 1 <= m <= 14:
            t[ord(ch)] = t[ord(ch.lower())] = m
    return t


def _seqs():
    """70 x 4133: samples 0 and 1 identical, 2 and 3 disjoint at every site, the rest a base sequence with SNPs, N, '-', lower case
    and every partial code sprinkled in; shorter alignments are its first L columns"""
    if "seqs" not in _CACHE:
        rng = np.random.default_rng(20250)
        L = max(LENGTHS)
        acgt = np.frombuffer(b"ACGT", np.uint8)
        base = acgt[rng.integers(0, 4, L)]
        seqs = np.tile(base, (N, 1))
        for s in range(4, N):
            hit = rng.random(L) < 0.02
            seqs[s, hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
            run = int(rng.integers(0, L - 200))
            hit = np.zeros(L, bool)
            hit[run:run + 200] = rng.random(200) < 0.25
            seqs[s, hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
            for chars, p in ((b"N-nx.", 0.02), (b"MRSVWYHKDB", 0.02), (b"mrsvwyhkdb", 0.005), (b"acgt", 0.03)):
                hit = rng.random(L) < p
                seqs[s, hit] = np.frombuffer(chars, np.uint8)[rng.integers(0, len(chars), int(hit.sum()))]
        seqs[1] = seqs[0]
        seqs[2] = np.frombuffer(b"AaMC", np.uint8)[rng.integers(0, 4, L)]          # masks within A | C
        seqs[3] = np.frombuffer(b"GtKT", np.uint8)[rng.integers(0, 4, L)]          # masks within G | T: disjoint from sample 2 everywhere
        seqs[5, :40] = ord("N")
        seqs.setflags(write=False)
        _CACHE["seqs"] = seqs
        _CACHE["masks"] = _mask_table()[seqs]
    return _CACHE["seqs"]


def _brute(masks, I, J):
    """-> (d per pair, sites, info) in list order, sites ascending within a pair: the definition on the masks"""
    snp = (masks[I] & masks[J]) == 0
    t, s = np.nonzero(snp)
    info = masks[I[t], s].astype(np.uint32) | (masks[J[t], s].astype(np.uint32) << 4)
    return snp.sum(1).astype(np.int64), s.astype(np.uint32), info


def _lists():
    iu = np.triu_indices(N, 1)
    every = (iu[0].astype(np.int32), iu[1].astype(np.int32))                        # all 2 415 pairs, row-major
    rng = np.random.default_rng(3)
    a = rng.integers(0, N, 150).astype(np.int32)
    b = ((a + 1 + rng.integers(0, N - 1, 150)) % N).astype(np.int32)                # never equal to a; i > j for about half
    assert (a != b).all() and (a > b).sum() > 30
    mixed = (np.concatenate([a, a[:40], [0, 1, 2, 3, 69, 64]]).astype(np.int32),    # duplicates, the identical pair, the disjoint pair
             np.concatenate([b, b[:40], [1, 0, 3, 2, 64, 69]]).astype(np.int32))
    return {"every": every, "mixed": mixed}


def _oracle_d(oracle, L):
    if ("od", L) not in _CACHE:
        r, c, d, _ = oracle.pairsnp_arrays(_seqs()[:, :L])
        mat = np.zeros((N, N), np.int64)
        mat[r.astype(np.int64), c.astype(np.int64)] = d.astype(np.int64)
        _CACHE["od", L] = mat + mat.T
    return _CACHE["od", L]


def _run(dev, aln, I, J, filter=False):
    import torch
    off, site, info = dev.pair_sites(aln, torch.from_numpy(np.ascontiguousarray(I, np.int32)).cuda(),
                                     torch.from_numpy(np.ascontiguousarray(J, np.int32)).cuda(), filter=filter)
    return off.cpu().numpy(), site.cpu().numpy().view(np.uint32), info.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("L", LENGTHS)
def test_sites_and_masks_equal_the_brute_force(oracle, hiplib, monkeypatch, L, form):
    from tracs_amd import device as dev
    monkeypatch.setenv("TRACS_PAIR_SITES_LANES_MIN", FORMS[form])
    seqs = _seqs()[:, :L]
    masks = _CACHE["masks"][:, :L]
    aln = dev.Alignment(N, L)
    aln.pack(np.ascontiguousarray(seqs))
    od = _oracle_d(oracle, L)
    try:
        for name, (I, J) in _lists().items():
            d, sites, info = _brute(masks, I, J)
            off, got_site, got_info = _run(dev, aln, I, J)
            assert off.dtype == np.int64 and np.array_equal(off, np.concatenate([[0], np.cumsum(d)])), (name, L, form)
            assert np.array_equal(d, od[I, J]), (name, L, form)
            assert np.array_equal(got_site, sites), (name, L, form)
            assert np.array_equal(got_info, info), (name, L, form)               # (bit 8 is never set without the filter)
            for t in range(0, len(I), 97):
                assert (np.diff(got_site[off[t]:off[t + 1]].astype(np.int64)) > 0).all()
            lo, hi = got_info & 15, (got_info >> 4) & 15
            assert ((lo & hi) == 0).all() and (lo != 15).all() and (hi != 15).all() and (lo != 0).all() and (hi != 0).all()
            if name == "mixed":
                k = len(I) - 6
                assert off[k + 1] == off[k] == off[k + 2] and off[k + 3] - off[k + 2] == L == off[k + 4] - off[k + 3]
        off, site, info = _run(dev, aln, np.zeros(0, np.int32), np.zeros(0, np.int32))       # m = 0
        assert off.tolist() == [0] and len(site) == 0 and len(info) == 0
    finally:
        aln.close()


def test_an_index_outside_the_alignment_is_refused(hiplib):
    from tracs_amd import device as dev
    L = 129
    aln = dev.Alignment(N, L)
    aln.pack(np.ascontiguousarray(_seqs()[:, :L]))
    try:
        with pytest.raises(RuntimeError, match="outside the alignment"):
            _run(dev, aln, np.array([0, 3], np.int32), np.array([1, N], np.int32))
    finally:
        aln.close()


# ---- verdicts ----------------------------------------------------------------------------------------------------------------------
def _fixture():
    if "fx" not in _CACHE:
        import make_pair_sites_golden as G
        with open(FIXTURE) as fh:
            fx = json.load(fh)
        _CACHE["fx"] = {L: [G.from_hex(p["flags"], p["d"]) for p in fx["pairs"] if p["L"] == L] for L in (9000, 120000)}
    return _CACHE["fx"]


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("variant", ["plain", "decorated"])
def test_verdicts_equal_the_definition_bit_for_bit(hiplib, monkeypatch, variant, form):
    """the crafted pairs (0, s) of tests/test_gpu_filter_hp.py: the sites are the crafted sites, the kept flags are the fixture's,
    and they sum to filter_recomb_pairs' filtered distance"""
    import torch
    import test_gpu_filter_hp as T
    from tracs_amd import device as dev
    monkeypatch.setenv("TRACS_PAIR_SITES_LANES_MIN", FORMS[form])
    for L, flags in _fixture().items():
        crafted = T._sites(L)
        assert len(crafted) == len(flags)
        seqs = T._alignment(L) if variant == "plain" else T._decorated(L)
        aln = dev.Alignment(seqs.shape[0], L)
        aln.pack(np.ascontiguousarray(seqs))
        try:
            J = np.arange(1, len(crafted) + 1, dtype=np.int32)
            I = np.zeros(len(J), np.int32)
            off, site, info = _run(dev, aln, I, J, filter=True)
            d = np.array([x[0] for x in crafted], np.int64)
            assert np.array_equal(np.diff(off), d), (L, variant, form)
            kept_sum = np.zeros(len(J), np.int64)
            for t, (dd, pos, expected) in enumerate(crafted):
                seg = slice(off[t], off[t + 1])
                assert np.array_equal(site[seg], pos.astype(np.uint32)), (L, t)
                kept = (info[seg] >> 8) == 0
                bad = np.nonzero(kept != flags[t])[0]
                assert not len(bad), (L, variant, form, t, int(dd), bad[:8].tolist())
                kept_sum[t] = int(kept.sum())
                assert kept_sum[t] == expected
            filt = dev.filter_recomb_pairs(aln, torch.from_numpy(I).cuda(), torch.from_numpy(J).cuda(),
                                           torch.from_numpy(d.astype(np.int32)).cuda()).cpu().numpy()
            assert np.array_equal(filt, kept_sum), (L, variant, form)
            assert ((info >> 9) == 0).all()
            plain = _run(dev, aln, I, J, filter=False)
            assert np.array_equal(plain[0], off) and np.array_equal(plain[1], site) and np.array_equal(plain[2], info & 0xFF)
        finally:
            aln.close()


def _planted():
    """70 x 20 000: a base sequence, a few SNPs per sample, and in every third sample a dense run that the filter removes"""
    if "planted" not in _CACHE:
        rng = np.random.default_rng(77)
        L = 20000
        acgt = np.frombuffer(b"ACGT", np.uint8)
        base = acgt[rng.integers(0, 4, L)]
        seqs = np.tile(base, (N, 1))
        for s in range(N):
            hit = rng.random(L) < 0.002
            seqs[s, hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
            if s % 3 == 0:
                start = int(rng.integers(0, L - 400))
                hit = np.zeros(L, bool)
                hit[start:start + 400] = rng.random(400) < 0.2
                seqs[s, hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
            hit = rng.random(L) < 0.01
            seqs[s, hit] = ord("N")
        _CACHE["planted"] = seqs
    return _CACHE["planted"]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_verdict_counts_equal_the_oracle(oracle, hiplib, monkeypatch, form):
    """every pair of a random alignment with planted dense runs: the rows number d, the kept ones the oracle's filtered distance"""
    from tracs_amd import device as dev
    monkeypatch.setenv("TRACS_PAIR_SITES_LANES_MIN", FORMS[form])
    seqs = _planted()
    if "planted_want" not in _CACHE:
        r, c, d, _ = oracle.pairsnp_arrays(seqs)
        _CACHE["planted_want"] = (r, c, d, oracle.filter_recomb_pairs(seqs, r, c, 4))
    r, c, d, filt = _CACHE["planted_want"]
    assert (filt < d).sum() > 100 and (filt > 0).sum() > 100
    aln = dev.Alignment(N, seqs.shape[1])
    aln.pack(seqs)
    try:
        off, site, info = _run(dev, aln, r.astype(np.int32), c.astype(np.int32), filter=True)
        assert np.array_equal(np.diff(off), d.astype(np.int64))
        kept = np.add.reduceat(((info >> 8) == 0).astype(np.int64), off[:-1][np.diff(off) > 0])
        assert np.array_equal(kept, filt.astype(np.int64)[np.diff(off) > 0])
    finally:
        aln.close()


# ---- rows: batches and the refusal -------------------------------------------------------------------------------------------------
def _write_rows(lib, h, I, J, path, filter=0, max_entries=10 ** 9, threads=4):
    from tracs_amd import _lib
    m = len(I)
    u32 = C.c_uint32 * max(m, 1)
    written = C.c_uint64(0)
    _lib.check(lib.tracs_distance_pair_sites(h, u32(*[int(x) for x in I]), u32(*[int(x) for x in J]), m, filter, max_entries, os.fsencode(path),
                                             None, None, 0, threads, C.byref(written)))
    return written.value


def test_rows_in_batches_and_the_refusal(hiplib, monkeypatch, tmp_path):
    from tracs_amd import _lib, synth
    L = 4133
    seqs = _seqs()
    masks = _CACHE["masks"]
    names = ["s%02d" % i for i in range(N)]
    fa = os.path.join(str(tmp_path), "aln.fa")
    synth.write_fasta(fa, np.array(seqs), names=names, width=80)
    I, J = _lists()["every"]
    I, J = np.concatenate([J[:100], I[:500]]), np.concatenate([I[:100], J[:500]])   # (the first 100 with i > j)
    d, sites, info = _brute(masks, I, J)
    total = int(d.sum())
    assert total > (1 << 18)                                                        # more than one formatting thread's slice
    lib = _lib.require_gpu()
    h = C.c_void_p()
    _lib.check(lib.tracs_distance_open((C.c_char_p * 1)(os.fsencode(fa)), 1, C.byref(h)))
    try:
        whole = os.path.join(str(tmp_path), "whole.csv")
        assert _write_rows(lib, h, I, J, whole, filter=1) == total
        text = open(whole).read()
        lines = text.split("\n")
        assert lines[0] == "sampleA,sampleB,contig,position,alleleA,alleleB,dropped" and lines[-1] == "" and len(lines) == total + 2
        t = np.repeat(np.arange(len(I)), d)
        for k in list(range(0, total, 997)) + [total - 1]:
            f = lines[1 + k].split(",")
            assert f[:6] == [names[I[t[k]]], names[J[t[k]]], "alignment", str(int(sites[k])), LETTERS[info[k] & 15], LETTERS[info[k] >> 4]], k
            assert f[6] in ("0", "1")
        monkeypatch.setenv("TRACS_PAIR_SITES_BATCH", str(total // 4))
        split = os.path.join(str(tmp_path), "split.csv")
        assert _write_rows(lib, h, I, J, split, filter=1, threads=1) == total
        assert open(split).read() == text
        monkeypatch.setenv("TRACS_PAIR_SITES_BATCH", "1")                           # every pair a batch of its own
        one = os.path.join(str(tmp_path), "one.csv")
        assert _write_rows(lib, h, I[:200], J[:200], one) == int(d[:200].sum())
        got = open(one).read().split("\n")
        assert len(got) == int(d[:200].sum()) + 2 and all(x.endswith(",NA") for x in got[1:-1])
        assert [x.rsplit(",", 1)[0] for x in got[1:-1]] == [x.rsplit(",", 1)[0] for x in lines[1:1 + int(d[:200].sum())]]
        monkeypatch.delenv("TRACS_PAIR_SITES_BATCH")
        refused = os.path.join(str(tmp_path), "refused.csv")
        with pytest.raises(RuntimeError, match=r"%d sites in all, more than --max-entries %d" % (total, total - 1)):
            _write_rows(lib, h, I, J, refused, max_entries=total - 1)
        assert not os.path.exists(refused)
        assert _write_rows(lib, h, I, J, refused, max_entries=total) == total
    finally:
        lib.tracs_distance_free(h)


def test_api_pair_sites_under_a_site_rule(hiplib, tmp_path):
    """api.pair_sites: names or indices, a keep bitmap -- the entries of the run on the alignment with the dropped columns deleted,
    and the positions that map them back"""
    from tracs_amd import api, synth
    from tracs_amd.sites import Sites
    L = 4133
    seqs, masks = _seqs(), _CACHE["masks"]
    names = ["s%02d" % i for i in range(N)]
    fa = os.path.join(str(tmp_path), "aln.fa")
    synth.write_fasta(fa, np.array(seqs), names=names, width=0)
    keep = np.ones(L, bool)
    keep[100:300] = keep[4000:] = False
    I, J = np.array([4, 69, 2, 0, 4], np.int32), np.array([68, 5, 3, 1, 68], np.int32)
    info = {}
    off, site, bits, got_names = api.pair_sites([fa], [("s04", 68), (69, "s05"), ("s02", "s03"), (0, 1), ("s04", "s68")], filter=True,
                                                sites=Sites(keep), info=info)
    d, sites, want = _brute(masks[:, keep], I, J)
    assert got_names == names and info["seqlen"] == int(keep.sum()) and np.array_equal(info["positions"], np.flatnonzero(keep))
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(d)])) and np.array_equal(site, sites) and np.array_equal(bits & 0xFF, want)
    assert d[2] == keep.sum() and d[3] == 0 and (bits >> 9 == 0).all() and (bits >> 8).any()
    with pytest.raises(ValueError, match="'nobody' is not among the samples"):
        api.pair_sites([fa], [("s04", "nobody")])
