"""Site rules on the host (tracs_amd/sites.py, the checks of `tracs distance`): BED parsing, contig offsets, keep bitmaps, the N-share
floor, the BED of the kept columns, every refusal before a GPU path, the new symbols -- and, on the CPU oracle, that the standard rule
of the GPU tests changes the results (a no-op implementation cannot pass them)."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

from site_rules_common import SIZES, is_n_table, standard_input, standard_rule


def _bed(tmp_path, text, name="m.bed"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_bed_comments_blank_lines_and_merging(tmp_path):
    from tracs_amd.sites import read_bed
    p = _bed(tmp_path, "# a comment\ntrack name=x\nbrowser position chr1:1-10\n\nchr1\t10\t20\tname\t0\t+\nchr1 15 30\n  \nchr1\t30\t31\nchr1\t100\t101\n"
                       "chr1\t5\t6\n")
    assert read_bed(p) == [(5, 6), (10, 31), (100, 101)]


@pytest.mark.parametrize("text,word", [
    ("chr1\t10\t10\n", "empty or reversed"),
    ("chr1\t10\t5\n", "empty or reversed"),
    ("chr1\t1\t5\nchr2\t1\t5\n", "--mask-reference"),
    ("chr1\t1\n", "expected contig, start, end"),
    ("chr1\ta\t5\n", "integers"),
])
def test_bed_errors_without_reference(tmp_path, text, word):
    from tracs_amd.sites import read_bed
    with pytest.raises(ValueError) as e:
        read_bed(_bed(tmp_path, text))
    assert word in str(e.value)


def _reference(tmp_path):
    p = tmp_path / "ref.fa"
    p.write_text(">c1 first contig\nACGTACGTAC\nACGTA\n>c2\nACGTACG\n")
    return str(p)


def test_contig_offsets_and_errors(tmp_path):
    from tracs_amd.align_post import read_contigs
    from tracs_amd.sites import contig_offsets, read_bed
    contigs = read_contigs(_reference(tmp_path))
    assert contigs == [("c1", 15), ("c2", 7)]
    assert contig_offsets(contigs) == {"c1": (0, 15), "c2": (15, 7)}
    assert read_bed(_bed(tmp_path, "c2\t0\t3\nc1\t13\t15\nc1\t2\t4\n"), contigs) == [(2, 4), (13, 18)]
    with pytest.raises(ValueError) as e:
        read_bed(_bed(tmp_path, "c3\t0\t3\n"), contigs)
    assert "'c3' is not in the reference" in str(e.value)
    with pytest.raises(ValueError) as e:
        read_bed(_bed(tmp_path, "c2\t0\t8\n"), contigs)
    assert "past the end of contig 'c2'" in str(e.value)


def test_keep_bitmap():
    from tracs_amd.sites import bitmap_to_bool, keep_bitmap
    L = 200
    w = keep_bitmap(L)
    assert w.dtype == np.uint64 and len(w) == 4 and bitmap_to_bool(w, L).all() and int(w[3]) == (1 << 8) - 1      # tail bits zero
    expect = np.zeros(L, bool); expect[10:70] = True; expect[130:131] = True
    assert np.array_equal(bitmap_to_bool(keep_bitmap(L, keep=[(10, 70), (130, 131)]), L), expect)
    assert int(keep_bitmap(L, keep=[(63, 65)])[0]) == 1 << 63 and int(keep_bitmap(L, keep=[(63, 65)])[1]) == 1
    m = np.ones(L, bool); m[0:3] = False; m[199:200] = False
    assert np.array_equal(bitmap_to_bool(keep_bitmap(L, mask=[(0, 3), (199, 200)]), L), m)
    both = expect.copy(); both[20:140] = False
    assert np.array_equal(bitmap_to_bool(keep_bitmap(L, keep=[(10, 70), (130, 131)], mask=[(20, 140)]), L), both)
    for kw in (dict(keep=[(0, 201)]), dict(mask=[(150, 201)])):
        with pytest.raises(ValueError) as e:
            keep_bitmap(L, **kw)
        assert "reaches past the alignment's length (200)" in str(e.value)


def test_max_n_samples_floors():
    from tracs_amd.sites import max_n_samples
    assert max_n_samples(0.2, 70) == 14 and max_n_samples(0.2, 131) == 26 and max_n_samples(0.2, 700) == 140
    assert max_n_samples(0.0, 10) == 0 and max_n_samples(0.999, 10) == 9 and max_n_samples(0.5, 3) == 1 and max_n_samples(0.1, 9) == 0


def test_kept_bed_round_trip(tmp_path):
    from tracs_amd.align_post import read_contigs
    from tracs_amd.sites import bool_to_bitmap, keep_bool, read_bed, write_kept_bed
    rng = np.random.default_rng(5)
    L = 22
    contigs = read_contigs(_reference(tmp_path))
    for trial in range(20):
        kept = rng.random(L) < 0.6
        kept[14:16] = trial % 2 == 0                       # a run across the contig boundary at 15
        for c in (None, contigs):
            for form in (kept, bool_to_bitmap(kept)):
                p = str(tmp_path / "kept.bed")
                write_kept_bed(p, form, L, c)
                assert np.array_equal(keep_bool(L, keep=read_bed(p, c)), kept)
    write_kept_bed(p, np.ones(L, bool), L, contigs)
    assert open(p).read() == "c1\t0\t15\nc2\t0\t7\n"
    write_kept_bed(p, np.ones(L, bool), L)
    assert open(p).read() == "alignment\t0\t22\n"


def _parser():
    from tracs_amd.distance import distance_parser
    return distance_parser(argparse.ArgumentParser())


REFUSALS = [
    (["--mask", "m.bed", "--gpus", "2"], ["one GPU", "--gpus 1"]),
    (["--keep", "m.bed", "--gpus", "2"], ["one GPU"]),
    (["--max-n-share", "0.2", "--gpus", "4"], ["one GPU"]),
    (["--sites-out", "k.bed"], ["--sites-out", "needs a site rule"]),
    (["--max-n-share", "1.0"], ["--max-n-share", "[0, 1)"]),
    (["--max-n-share", "-0.1"], ["--max-n-share", "[0, 1)"]),
    (["--max-n-share", "nan"], ["--max-n-share", "[0, 1)"]),
    (["--mask-reference", "ref.fa"], ["--mask-reference", "--mask or --keep"]),
    (["--mask-reference", "ref.fa", "--max-n-share", "0.2"], ["--mask-reference", "--mask or --keep"]),
]


@pytest.mark.parametrize("extra,words", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_refusals_before_any_gpu_path(tmp_path, monkeypatch, extra, words):
    import tracs_amd.distance as di
    from tracs_amd import _lib, multigpu

    def no_gpu(*a, **k):
        raise AssertionError("a GPU path was entered or the library was loaded")
    monkeypatch.setattr(multigpu, "spawn", no_gpu)
    monkeypatch.setattr(multigpu, "init", no_gpu)
    for name in ("nearest_arrays", "pairsnp_arrays", "_rows_on_device", "_forest_on_device", "_histogram_on_device"):
        monkeypatch.setattr(di, name, no_gpu)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(_lib, "load", no_gpu)
    out = tmp_path / "o.csv"
    a = _parser().parse_args(["--msa", "x.fa", "-o", str(out)] + extra)
    with pytest.raises(SystemExit) as e:
        a.func(a)
    msg = str(e.value.code)
    assert msg.startswith("tracs distance: ")
    for w in words:
        assert w in msg, (w, msg)
    assert not os.path.exists(out)


def test_parser_defaults_and_bed_past_the_end(tmp_path, monkeypatch):
    import tracs_amd.distance as di
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.csv"])
    assert a.mask_bed is None and a.keep_bed is None and a.mask_reference is None and a.max_n_share is None and a.sites_out is None
    di.check_site_args(a)
    assert di.site_rule_for(["x.fa"], a, di.read_site_files(a)) is None          # no option: no rule, no file touched
    fa = tmp_path / "a.fa"
    fa.write_text(">s0\nACGTACGTAC\nAC\n>s1\nACGTACGTACAC\n")
    a = _parser().parse_args(["--msa", str(fa), "-o", "o.csv", "--mask", _bed(tmp_path, "x\t3\t5\n")])
    rule = di.site_rule_for([str(fa)], a, di.read_site_files(a))
    assert rule.L == 12 and rule.max_n is None and rule.keep.tolist() == [True] * 3 + [False] * 2 + [True] * 7
    a = _parser().parse_args(["--msa", str(fa), "-o", "o.csv", "--mask", _bed(tmp_path, "x\t3\t13\n")])
    with pytest.raises(SystemExit) as e:
        di.site_rule_for([str(fa)], a, di.read_site_files(a))
    assert "reaches past the alignment's length (12)" in str(e.value.code) and str(fa) in str(e.value.code)


def test_new_symbols(hiplib):
    from tracs_amd import _lib
    names = ["tracs_alignment_site_n_counts", "tracs_alignment_select_sites", "tracs_pairsnp_sites", "tracs_nearest_sites",
             "tracs_distance_open_sites", "tracs_distance_source_len", "tracs_distance_len", "tracs_distance_kept_sites"]
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(hiplib, name), name
    vp, sz, u64p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)
    assert hiplib.tracs_alignment_select_sites.argtypes == [vp, u64p, sz, C.c_uint32, C.POINTER(vp), u64p, C.POINTER(sz), vp]
    assert hiplib.tracs_alignment_site_n_counts.argtypes == [vp, vp, vp]
    assert hiplib.tracs_alignment_site_n_counts(None, None, None) == -1
    out = vp()
    assert hiplib.tracs_alignment_select_sites(None, None, 0, 0xFFFFFFFF, C.byref(out), None, None, None) == -1
    assert hiplib.tracs_distance_source_len(None) == 0 and hiplib.tracs_distance_len(None) == 0
    assert hiplib.tracs_abi_version() == 1
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"site_n_count_kernel" in blob and b"select_sites_kernel" in blob


@pytest.mark.parametrize("n,L", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_standard_rule_changes_the_results(oracle, hiplib, n, L):
    """What the GPU tests rely on, on the CPU oracle: the N rule drops exactly the run columns, the kept count is no multiple of 128,
    and d, nn and the filtered distance of the column-deleted alignment differ from the unmasked ones nearly everywhere."""
    isn = is_n_table(hiplib)
    seqs, runs = standard_input(n, L)
    keep, max_n, kept = standard_rule(seqs, isn)
    assert max_n == (14, 26, 140)[SIZES.index((n, L))]
    assert np.array_equal((isn[seqs].sum(axis=0) > max_n), runs)
    assert kept.sum() % 128 != 0 and kept.sum() == L - 458 - runs.sum()
    r, c, d, nn = oracle.pairsnp_arrays(seqs)
    rk, ck, dk, nnk = oracle.pairsnp_arrays(seqs[:, kept])
    assert np.array_equal(r, rk) and np.array_equal(c, ck)
    assert (d != dk).mean() > 0.98
    assert (nn != nnk).all()
    if n <= 131:
        f, fk = oracle.filter_recomb_pairs(seqs, r, c, 4), oracle.filter_recomb_pairs(seqs[:, kept], r, c, 4)
    else:                                  # (the filter on 244 650 pairs is the slow part: every 20th pair)
        f, fk = oracle.filter_recomb_pairs(seqs, r[::20], c[::20], 4), oracle.filter_recomb_pairs(seqs[:, kept], r[::20], c[::20], 4)
    assert (f != fk).mean() > 0.94
