"""The sample and pair rules on the host: the flags, every refusal before a GPU path and its message, the
--samples-out writer, the numpy expectation the GPU tests compare against (on a hand-made alignment), the planted cases of the
standard input, and the new symbols."""
import argparse
import math
import os
import re

import numpy as np
import pytest

from sample_rules_common import F, G, check_plan, expected, planted_input
from site_rules_common import is_n_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(*extra):
    from tracs_amd.distance import distance_parser
    return distance_parser(argparse.ArgumentParser()).parse_args(["--msa", "a.fa", "-o", "out.csv"] + list(extra))


def test_parser_accepts_the_flags():
    a = _args("--max-sample-n-share", "0.6", "--min-sites", "1200", "--samples-out", "s.csv")
    assert a.max_sample_n_share == 0.6 and a.min_sites == 1200 and a.samples_out == "s.csv"
    a = _args()
    assert a.max_sample_n_share is None and a.min_sites is None and a.samples_out is None


@pytest.mark.parametrize("extra,message", [
    (["--max-sample-n-share", "1.5"], "--max-sample-n-share must be in [0, 1], got 1.5"),
    (["--max-sample-n-share", "-0.1"], "--max-sample-n-share must be in [0, 1], got -0.1"),
    (["--max-sample-n-share", "nan"], "--max-sample-n-share must be in [0, 1], got nan"),
    (["--min-sites", "0"], "--min-sites must be in [1, 2^32 - 1], got 0"),
    (["--min-sites", "-3"], "--min-sites must be in [1, 2^32 - 1], got -3"),
    (["--samples-out", "s.csv"], "--samples-out needs --max-sample-n-share (it lists what the sample rule decided)"),
    (["--samples-out", "s.csv", "--min-sites", "5"], "--samples-out needs --max-sample-n-share (it lists what the sample rule decided)"),
    (["--max-sample-n-share", "0.5", "--gpus", "2"],
     "the sample and pair rules (--max-sample-n-share, --min-sites) run on one GPU; use --gpus 1"),
    (["--min-sites", "5", "--gpus", "2"], "the sample and pair rules (--max-sample-n-share, --min-sites) run on one GPU; use --gpus 1"),
])
def test_refusals_before_the_gpu(extra, message):
    from tracs_amd.distance import check_sample_args
    with pytest.raises(SystemExit) as e:
        check_sample_args(_args(*extra))
    assert str(e.value) == "tracs distance: " + message


def test_samples_out_with_several_msa_is_refused():
    from tracs_amd.distance import check_sample_args, distance_parser
    a = distance_parser(argparse.ArgumentParser()).parse_args(["--msa", "a.fa", "b.fa", "-o", "o.csv", "--max-sample-n-share", "0.5",
                                                               "--samples-out", "s.csv"])
    with pytest.raises(SystemExit) as e:
        check_sample_args(a)
    assert str(e.value) == "tracs distance: --samples-out describes one alignment; give one --msa file"


def test_accepted_combinations_pass_the_check():
    from tracs_amd.distance import check_sample_args
    for extra in ([], ["--max-sample-n-share", "0"], ["--max-sample-n-share", "1", "--samples-out", "s.csv"], ["--min-sites", "1"],
                  ["--max-sample-n-share", "0.5", "--min-sites", "4294967295", "--nearest", "3"]):
        check_sample_args(_args(*extra))


def test_refused_before_anything_is_opened(tmp_path):
    """the whole command: the refusal comes before the output file is created or a library is loaded"""
    from tracs_amd.distance import distance
    out = tmp_path / "o.csv"
    a = _args("--min-sites", "0")
    a.output_file = str(out)
    with pytest.raises(SystemExit) as e:
        distance(a)
    assert "--min-sites" in str(e.value) and not out.exists()


def test_samples_out_writer(tmp_path):
    from tracs_amd.distance import SAMPLES_HEADER, write_samples_out
    p = tmp_path / "s.csv"
    write_samples_out(str(p), ["a", "b c", "d"], "ref1", np.array([0, 17, 4], np.uint32), 120, [True, 0, 1])
    assert SAMPLES_HEADER == "sample,MSA file,N sites,sites,kept\n"
    assert p.read_text() == SAMPLES_HEADER + "a,ref1,0,120,1\nb c,ref1,17,120,0\nd,ref1,4,120,1\n"


def test_api_refuses_bad_rule_arguments():
    """the keyword checks of the array entry points come before the library is asked for a GPU"""
    from tracs_amd.handle import rules_struct
    from tracs_amd.sites import Sites
    with pytest.raises(ValueError, match="max_sample_n_share must be in"):
        rules_struct(None, 1.2, None, None)
    with pytest.raises(ValueError, match="max_n_share must be in"):
        rules_struct(None, None, -0.5, None)
    with pytest.raises(ValueError, match="min_sites must be in"):
        rules_struct(None, None, None, 0)
    with pytest.raises(ValueError, match="cannot be combined with max_sample_n_share"):
        rules_struct(Sites(max_n_samples=3), 0.5, None, None)
    with pytest.raises(ValueError, match="two forms of one rule"):
        rules_struct(Sites(max_n_samples=3), None, 0.2, None)
    r, alive = rules_struct(Sites(max_n_samples=3), None, None, None)                      # the threshold travels as it is
    assert alive is None and not r.keep and (r.keep_len, r.max_n_share, r.max_sample_n_share, r.min_sites, r.max_n_samples) == (0, -1.0, -1.0, 0, 3)
    r, alive = rules_struct(None, None, None, None)                                        # nothing given: no field set
    assert alive is None and not r.keep and (r.keep_len, r.max_n_share, r.max_sample_n_share, r.min_sites, r.max_n_samples) == (0, -1.0, -1.0, 0, 0xFFFFFFFF)
    r, alive = rules_struct(Sites(np.array([True, False, True])), 0.5, 0.25, 7)
    assert (r.keep_len, r.max_n_share, r.max_sample_n_share, r.min_sites, r.max_n_samples) == (3, 0.25, 0.5, 7, 0xFFFFFFFF)
    assert int(alive[0]) == 0b101
    r, alive = rules_struct(None, None, None, 9)
    assert not r.keep and (r.max_n_share, r.max_sample_n_share, r.min_sites) == (-1.0, -1.0, 9)


def test_expectation_on_a_hand_made_alignment(hiplib):
    isn = is_n_table(hiplib)
    rows = [b"ACGTACGTACGT",       # no N
            b"NNNNACGTACGT",       # 4 N, 3 of them under the bitmap below
            b"ACGTNN-TACGT",       # 3 N ('-' counts)
            b"RCGTNCGTACGN",       # 2 N (R is a partial code, not N)
            b"NNNNNNNNACGT",       # 8 N
            b"acgtnCGTACGT"]       # 1 N (lower case n)
    seqs = np.frombuffer(b"".join(rows), np.uint8).reshape(6, 12).copy()
    e = expected(seqs, isn, None, 0.25, None)                                         # T = floor(0.25 * 12) = 3
    assert e["rule_sites"] == 12 and e["threshold"] == 3
    assert e["n_counts"].tolist() == [0, 4, 3, 2, 8, 1] and e["kept_samples"].tolist() == [True, False, True, True, False, True]
    assert e["kept_sites"].all()
    keep = np.ones(12, bool)
    keep[0] = keep[11] = False                                                        # L' = 10, T = floor(0.25 * 10) = 2
    e = expected(seqs, isn, keep, 0.25, 0.25)
    assert e["rule_sites"] == 10 and e["threshold"] == 2
    assert e["n_counts"].tolist() == [0, 3, 3, 1, 7, 1] and e["kept_samples"].tolist() == [True, False, False, True, False, True]
    # the N share over the three survivors: floor(0.25 * 3) = 0 -> a column stays only if none of rows 0, 3, 5 is N there
    assert e["kept_sites"].tolist() == [False] + [True] * 3 + [False] + [True] * 6 + [False]
    # ... over all six it would be floor(1.5) = 1, and column 5 (N in rows 2 and 4, both dropped) would have gone: the order matters
    all_six = keep & (isn[seqs].sum(axis=0) <= 1)
    assert e["kept_sites"][5] and not all_six[5]
    e = expected(seqs, isn, None, 1.0, None)                                          # G = 1 drops nothing
    assert e["kept_samples"].all()
    e = expected(seqs, isn, None, 0.0, None)                                          # G = 0: only records without any N stay
    assert e["kept_samples"].tolist() == [True, False, False, False, False, False]


@pytest.mark.parametrize("n,L,n_query,with_files", [(70, 5000, None, True), (70, 5000, 25, True), (70, 5000, None, False), (131, 30001, None, True)])
def test_planted_cases_are_what_they_claim(hiplib, n, L, n_query, with_files):
    isn = is_n_table(hiplib)
    seqs, keep, plan = planted_input(n, L, isn, n_query=n_query, with_files=with_files)
    e = check_plan(seqs, isn, keep, plan, n_query)
    assert e["threshold"] == math.floor(G * e["rule_sites"])
    assert (keep is None) == (not with_files) and 0.0 < F < G


def _declared():
    text = open(os.path.join(ROOT, "include", "tracs_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(tracs_[a-z_A-Z0-9]+)\s*\(", text))


NEW_SYMBOLS = ["tracs_alignment_sample_n_counts", "tracs_alignment_select_samples", "tracs_pairs_min_sites", "tracs_pairsnp_rules",
               "tracs_nearest_rules", "tracs_distance_open_rules"] + \
              ["tracs_%s_%s" % (k, a) for k in ("pairsnp", "distance") for a in ("source_nseq", "source_name", "source_n_count", "source_kept",
                                                                                 "rule_sites")]


def test_new_symbols_are_declared_bound_and_exported(hiplib):
    from tracs_amd import _lib
    declared = _declared()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        f = getattr(hiplib, name)
        assert f.argtypes is not None, name
    assert hiplib.tracs_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "tracs_hip.h")).read()
    assert "typedef struct tracs_rules" in header
    for field in ("keep", "keep_len", "max_n_share", "max_sample_n_share", "min_sites"):
        assert re.search(r"\b%s;" % field, header), field


def test_argument_errors_do_not_need_a_gpu(hiplib):
    import ctypes as C
    from tracs_amd import _lib
    h = C.c_void_p()
    one = (C.c_char_p * 1)(b"nope.fa")
    for share in (1.5, float("nan")):
        r = _lib.Rules(None, 0, -1.0, share, 0, 0xFFFFFFFF)
        assert hiplib.tracs_pairsnp_rules(one, 1, 1, 10, 0, C.byref(r), C.byref(h)) == -1
        assert hiplib.tracs_last_error() == b"tracs_rules: a share must be in [0, 1], or negative for no rule"
    r = _lib.Rules(None, 0, 0.2, -1.0, 0, 5)
    assert hiplib.tracs_distance_open_rules(one, 1, C.byref(r), C.byref(h)) == -1
    assert b"two forms of one rule" in hiplib.tracs_last_error()
    assert hiplib.tracs_alignment_sample_n_counts(None, None, 0, None, None) == -1
    assert hiplib.tracs_last_error() == b"tracs_alignment_sample_n_counts: NULL argument"
    assert hiplib.tracs_alignment_select_samples(None, None, C.byref(h), None) == -1
    assert hiplib.tracs_last_error() == b"tracs_alignment_select_samples: NULL argument"
    assert hiplib.tracs_pairs_min_sites(None, None, 8, 8, 0, 8, 0, 10, 3, None) == -1
    assert hiplib.tracs_last_error() == b"tracs_pairs_min_sites: NULL argument"
    assert hiplib.tracs_pairs_min_sites(None, None, 8, 8, 0, 8, 0, 10, 0, None) == 0      # no rule: nothing to do, nothing read
