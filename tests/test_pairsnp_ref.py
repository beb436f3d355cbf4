"""The oracle's pair loop and recombination filter against the reference's own source: src/pairsnp.hpp compiled unmodified over
oracle/boost_standin (oracle/_ref/_tracs_ref_pairsnp), its outputs stored in tests/golden/pairsnp_ref_golden.npz (generator:
tests/golden/make_golden.py pairsnp-ref) and, where oracle/_ref is present, the module itself.  The checks live in
tests/pairsnp_ref_check.py and run as child processes (the reference's build flags switch a process to flush-to-zero).

What is the reference's here: load_seqs (the IUPAC switch, its default branch, toupper), the pair loop, d <= dist, the two-file
j_start, the output order, range_count, filter_recomb's windows and clamps.  What is ours: the bitset's members (checked below
against std::vector<bool> under ASan + UBSan) and the binomial CDF's numerics (held to the definition at 50 digits: `cdf`).

Mutation check (run once by hand, not part of the suite): with `d <= dist` turned into `d < dist` in orc_pairsnp, or with 'R'
given the mask of 'M' in orc_iupac_mask, test_oracle_pair_loop_and_filter_equal_the_reference fails (first at iupac_small/thr: 3 pairs
for 8; first at iupac_small/all: 7 of 21 distances)."""
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)


def _child(section):
    out = subprocess.run([sys.executable, os.path.join(HERE, "pairsnp_ref_check.py"), section], capture_output=True, text=True,
                         timeout=900, cwd=ROOT)
    assert out.returncode == 0 and ("OK " + section) in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    print(out.stdout.strip())
    ref = os.path.join(ROOT, "oracle", "_ref")
    if os.path.isdir(ref) and any(f.startswith("_tracs_ref_pairsnp") for f in os.listdir(ref)):
        assert "live" in out.stdout and "skipped" not in out.stdout, out.stdout     # where the reference was built, it is compared
    return out.stdout


def test_fixture_is_self_contained_and_covers_the_cases():
    import numpy as np
    import pairsnp_ref_cases as PC
    meta, arrays = PC.load()
    golden = os.path.join(HERE, "golden")
    assert os.path.getsize(PC.FIXTURE) <= max(os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden)
                                              if f != os.path.basename(PC.FIXTURE))
    cases = {c["name"]: c for c in meta["cases"] + meta["filter_cases"]}
    assert len(cases) == len(meta["cases"]) + len(meta["filter_cases"])
    for c in cases.values():
        seqs = arrays["aln/" + c["aln"]]
        assert seqs.dtype == np.uint8 and seqs.ndim == 2
        r, cc, d, nn, filt = PC.expected(arrays, c)
        assert len(r) == len(cc) == len(d) == len(nn) == len(filt)
        assert (d <= c["dist"]).all() and (nn <= seqs.shape[1]).all() and (r < cc).all()
    for name in ("iupac_small", "tail_129", "consensus_300"):
        assert all("%s/%s" % (name, m) in cases for m in ("all", "thr", "twofile"))
    by = set(arrays["aln/bytes"].reshape(-1).tolist())
    assert by >= set(range(33, 127)) - set(b">+@") and not by & set(b">+@")
    assert {arrays["aln/len_%d" % L].shape[1] for L in (1, 63, 64, 65, 127, 128, 129)} == {1, 63, 64, 65, 127, 128, 129}
    assert arrays["aln/n70"].shape == (70, 4133) and arrays["aln/n130"].shape == (130, 1000)
    for key in ("n70", "n130"):
        a = arrays["aln/" + key]
        assert (a == ord("N")).any() and np.isin(a, np.frombuffer(b"MRWSYKVHDB", np.uint8)).any() and ((a >= 97) & (a <= 122)).any()
    assert (arrays["aln/identical"] == arrays["aln/identical"][0]).all() and not arrays["identical/all/d"].any()
    assert (arrays["all_differ/all/d"] == 130).sum() == 9 and (arrays["all_differ/all/d"] == 0).sum() == 1
    assert (arrays["aln/all_n"][2] == ord("N")).all() and not arrays["all_n/all/nn"][arrays["all_n/all/cols"] == 2].any()
    D = meta["dist_d"]
    full = arrays["n130/all/d"]
    assert D in full and [cases["n130/" + t]["dist"] for t in ("dist_minus1", "dist_0", "dist_d", "dist_d_minus1")] == [-1, 0, D, D - 1]
    assert [len(arrays["n130/%s/d" % t]) for t in ("dist_minus1", "dist_0", "dist_d", "dist_d_minus1")] == \
        [0, int((full <= 0).sum()), int((full <= D).sum()), int((full < D).sum())]
    assert (full <= 0).any() and cases["n130/all"]["dist"] == PC.INT_MAX
    assert [cases["n130/n0_%d" % k]["n0"] for k in (1, 43, 129)] == [1, 43, 129]
    assert cases["tail_129/wrapped"]["width"] and cases["tail_129/crlf"]["crlf"] and cases["tail_129/gz"]["gz"]
    assert sorted(c["aln"] for c in meta["filter_cases"] if c["dist"] == PC.INT_MAX) == ["filter_dense_one", "filter_end", "filter_lineage"]
    assert not arrays["filter_dense_one/unfiltered/filt"].any() and len(arrays["filter_dense_one/unfiltered/filt"]) == 28
    assert meta["margin"] == 1e-9 and meta["measured"]["ill_cells"] == 0 and meta["measured"]["min_relative_margin"] > meta["margin"]
    assert arrays["hp/ref"].shape == (25, 3)


def test_oracle_pair_loop_and_filter_equal_the_reference():
    _child("pairloop")


def test_oracle_filter_positions_equal_the_reference_and_the_definition():
    pytest.importorskip("mpmath")
    _child("positions")


def test_standin_cdf_within_the_oracles_bound_of_the_definition():
    pytest.importorskip("mpmath")
    _child("cdf")


def test_reference_range_count_is_the_span_and_the_count():
    _child("range_count")


def test_standin_bitset_against_vector_bool_under_sanitizers(tmp_path):
    """every member of oracle/boost_standin/boost/dynamic_bitset.hpp the reference uses, at sizes 0, 1, 63, 64, 65, 128 and 1000: a
    stand-alone program under ASan + UBSan"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the bitset check"
    exe = os.path.join(str(tmp_path), "test_dynamic_bitset")
    src = os.path.join(ROOT, "oracle", "boost_standin", "test_dynamic_bitset.cpp")
    cc = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I" + os.path.join(ROOT, "oracle", "boost_standin"), "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "bitset ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
