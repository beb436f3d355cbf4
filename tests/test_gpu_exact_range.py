"""The exact-sum bounds of the matrix-core pair kernels on alignments longer than one exact range.

pairsnp_mfma_kernel (consensus, general, count) keeps its sums in fp32 accumulators; the results are exact because the host never
gives one workgroup a site range whose partial sum could reach 2^24 (csrc/pairsnp.hip: max_gps in pairs_one_launch, thr_prefix_groups
and thr_remainder_split, 2^16 groups in count_pass).  Here the bound alone splits the range: a handful of samples (one tile), lengths
beyond the bounds -- 3 x 2^21 + 77 sites for the pair kernels, 2^24 + 2^21 + 77 for the counting pass --, TRACS_KSPLIT=1 so that nothing
else cuts the range, and in every case one pair whose sum over the whole alignment passes 2^24 (asserted from the reference).  Every
comparison is exact equality of d and nn over all pairs against a plain int64 reference on the 4-bit allele sets, which must agree
with the oracle first.  tests/test_fp32_range_model.py shows on the CPU that these inputs come out wrong when a range runs over the
whole alignment.  The pair-kernel tests switch the site classes off: the pair kernel then reads every site.

Inputs: tests/exact_range_cases.py.  n = 6 (consensus), n = 14 (general: the six rows and eight copies of row 0, without which the general
route refuses its lists and the VALU kernel runs), n = 3 (count: the site classes take it as it is).

Measured on an MI355X: the dense calls alone (the first one of a handle includes the once-per-pack work), and the whole test with
its inputs, reference and oracle (built once per case and shared; each child process starts Python anew and builds its own):

    test_one_launch[consensus]              TRACS_KSPLIT=1 22.7 ms, default 19.7 ms, TRACS_KSPLIT=2 19.6 ms        2.2 s
    test_one_launch[general]                TRACS_KSPLIT=1 52.8 ms, default 6.7 ms                                 1.2 s
    test_thresholded_two_pass[consensus]    default prefix 6.9 ms, TRACS_THR_PREFIX=49152 26.6 ms                  0.04 s
    test_thresholded_two_pass[general]      default prefix 43.4 ms, TRACS_THR_PREFIX=49152 34.7 ms                 0.08 s
    test_count_pass_in_place                20.4 ms                                                                2.8 s
    test_count_pass_repacked                19.7 ms                                                                2.7 s
    test_valu_control[consensus]            70.4 ms                                                                2.8 s
    test_valu_control[general]              103.9 ms                                                               3.5 s

On the same GPU, the same calls against a library built without the bounds (max_gps = groups, no 2^16-group bound in count_pass), with
TRACS_KSPLIT=1: consensus d(0, 1), d(0, 2), d(1, 2) off by -2831, -3080, -3054; general d(4, 5) off by -43; count nn(1, 2) off by +3706 in
place and -2 re-packed.  With the parent's thr_prefix_groups (a forced prefix not held to max_gps) TRACS_THR_PREFIX=49152 gave consensus
d(0, 2), d(1, 2) off by -3080, -3054 and general d(4, 5) off by -38; everything else was exact.
"""
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import exact_range_cases as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = {"consensus": "mfma", "general": "mfma-general"}


@functools.lru_cache(maxsize=None)
def _inputs(kind):
    """-> seqs, reference d, nn (int64, X.pairs order): built once, shared, never changed"""
    seqs = X.BUILDERS[kind]()
    seqs.setflags(write=False)
    d, nn = X.reference(seqs)
    d.setflags(write=False); nn.setflags(write=False)
    return seqs, d, nn


@functools.lru_cache(maxsize=None)
def _case(kind, oracle):
    seqs, d, nn = _inputs(kind)
    X.assert_precondition(kind, seqs)
    er, ec, ed, enn = oracle.pairsnp_arrays(seqs, n_threads=8)
    ri, ci = X.pairs(len(seqs))
    assert np.array_equal(er.astype(np.int64), ri) and np.array_equal(ec.astype(np.int64), ci)
    assert np.array_equal(ed.astype(np.int64), d) and np.array_equal(enn.astype(np.int64), nn), "the reference and the oracle disagree"
    return seqs, ri, ci, d, nn


@pytest.fixture
def every_site_dense(hiplib):
    """no site classes: the pair kernel reads the whole alignment"""
    hiplib.tracs_debug_force_site_classes(0)
    yield
    hiplib.tracs_debug_force_site_classes(-2)


def _packed(seqs):
    import torch
    from tracs_amd import device as dev
    n, L = seqs.shape
    aln = dev.Alignment(n, L)
    aln.pack(seqs)
    return aln, torch.empty((n, n), dtype=torch.int32, device="cuda"), torch.empty((n, n), dtype=torch.int32, device="cuda")


def _dense(aln, d, nn, **kw):
    """one dense call into poisoned cells -> its duration in ms"""
    import torch
    from tracs_amd import device as dev
    d.fill_(-7); nn.fill_(-7)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev.pairsnp_dense(aln, d, nn, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


@pytest.mark.parametrize("kind", ["consensus", "general"])
def test_one_launch(kind, hiplib, oracle, monkeypatch, every_site_dense):
    """pairs_one_launch: with TRACS_KSPLIT=1 the bound alone splits the range; the default split; and (consensus) TRACS_KSPLIT=2, whose
    ranges of 3 x 2^20 sites stay under the bound"""
    seqs, ri, ci, ref_d, ref_nn = _case(kind, oracle)
    aln, d, nn = _packed(seqs)
    for ksplit in ("1", None) + (("2",) if kind == "consensus" else ()):
        if ksplit is None:
            monkeypatch.delenv("TRACS_KSPLIT", raising=False)
        else:
            monkeypatch.setenv("TRACS_KSPLIT", ksplit)
        ms = _dense(aln, d, nn)
        print("%s one launch, TRACS_KSPLIT=%s: %.1f ms" % (kind, ksplit, ms))
        assert aln.encoding == kind and aln.kernel == KERNEL[kind] and aln.site_classes is None
        assert np.array_equal(d.cpu().numpy()[ri, ci].astype(np.int64), ref_d), (kind, ksplit)
        assert np.array_equal(nn.cpu().numpy()[ri, ci].astype(np.int64), ref_nn), (kind, ksplit)
    aln.close()


@pytest.mark.parametrize("kind", ["consensus", "general"])
def test_thresholded_two_pass(kind, hiplib, oracle, monkeypatch, every_site_dense):
    """pairs_two_pass: the default prefix, and TRACS_THR_PREFIX forced to the largest whole-stage value below the alignment's groups
    (49 152: the whole general pair (4, 5), G ~ 20 M, in what would be ONE prefix range -- thr_prefix_groups must hold a forced value
    to the bound as it holds the default).  Pairs within the threshold: d and nn exact; the others beyond it or negative."""
    seqs, ri, ci, ref_d, ref_nn = _case(kind, oracle)
    at = {p: k for k, p in enumerate(zip(ri.tolist(), ci.tolist()))}
    thr = int(ref_d[at[1, 2]]) if kind == "consensus" else int(max(ref_d[at[1, 2]], ref_d[at[4, 5]]))
    keep = ref_d <= thr
    assert keep[at[X.NAMED_PAIR[kind]]] and not keep.all()
    monkeypatch.delenv("TRACS_KSPLIT", raising=False)
    aln, d, nn = _packed(seqs)
    for prefix in (None, X.forced_prefix(kind)):
        if prefix is None:
            monkeypatch.delenv("TRACS_THR_PREFIX", raising=False)
        else:
            assert prefix == 49152 and prefix < X.groups_of(seqs.shape[1])
            monkeypatch.setenv("TRACS_THR_PREFIX", str(prefix))
        ms = _dense(aln, d, nn, dist_threshold=thr)
        print("%s two-pass, TRACS_THR_PREFIX=%s: %.1f ms" % (kind, prefix, ms))
        assert aln.encoding == kind and aln.kernel == KERNEL[kind] and aln.site_classes is None
        dh, nh = d.cpu().numpy()[ri, ci].astype(np.int64), nn.cpu().numpy()[ri, ci].astype(np.int64)
        assert np.array_equal(dh[keep], ref_d[keep]), (kind, prefix, dh, ref_d)
        assert np.array_equal(nh[keep], ref_nn[keep]), (kind, prefix, nh, ref_nn)
        assert ((dh[~keep] > thr) | (dh[~keep] < 0)).all(), (kind, prefix)
    aln.close()


# ---- switches read once per process: one child each -----------------------------------------------------------------------------
CHILD = r'''
import json, sys, time
import numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import exact_range_cases as X
from oracle import oracle as O
from tracs_amd import device as dev
kind = sys.argv[1]
seqs = X.BUILDERS[kind]()
pre = X.assert_precondition(kind, seqs)
ref_d, ref_nn = X.reference(seqs)
er, ec, ed, enn = O.pairsnp_arrays(seqs, n_threads=8)
ri, ci = X.pairs(len(seqs))
assert np.array_equal(er.astype(np.int64), ri) and np.array_equal(ec.astype(np.int64), ci)
assert np.array_equal(ed.astype(np.int64), ref_d) and np.array_equal(enn.astype(np.int64), ref_nn), "the reference and the oracle disagree"
n, L = seqs.shape
aln = dev.Alignment(n, L)
aln.pack(seqs)
d = torch.full((n, n), -7, dtype=torch.int32, device="cuda"); nn = torch.full((n, n), -7, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
t0 = time.perf_counter()
dev.pairsnp_dense(aln, d, nn)
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) * 1e3
isn = X.MASK_OF[seqs] == 15
print("RESULT " + json.dumps({
    "encoding": aln.encoding, "kernel": aln.kernel, "classes": aln.site_classes, "count_source": aln.count_source, "ms": ms, "sum": pre,
    "sites_with_two_n": int(np.count_nonzero(isn.sum(axis=0) >= 2)), "L": L,
    "d": d.cpu().numpy()[ri, ci].tolist(), "nn": nn.cpu().numpy()[ri, ci].tolist(), "ref_d": ref_d.tolist(), "ref_nn": ref_nn.tolist()}))
aln.close()
'''


def _child(kind, env):
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}, kind], capture_output=True, text=True,
                         env=dict(os.environ, **env), timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print("%s %s: dense call %.1f ms, named pair's sum %d, %s, classes %s, count source %s" %
          (kind, env, r["ms"], r["sum"], r["kernel"], r["classes"], r["count_source"]))
    return r


def _count_pass(in_place):
    r = _child("count", {"TRACS_SITE_CLASSES": "1", "TRACS_NN_LISTS": "0", "TRACS_COUNT_IN_PLACE": "1" if in_place else "0", "TRACS_KSPLIT": "1"})
    assert r["classes"] is not None and r["classes"][0] == 0, r["classes"]       # on site classes, no dense site: the counting pass makes every nn
    assert r["encoding"] == "consensus" and r["kernel"] == "mfma"
    # the source asked for: every site in place / the sites with a pair of N samples re-packed; nothing from lists
    assert r["count_source"] == [r["L"] if in_place else r["sites_with_two_n"], in_place, 0], r["count_source"]
    assert r["count_source"][0] > X.BOUND_SITES["count"]
    assert r["nn"] == r["ref_nn"], (r["nn"], r["ref_nn"])
    assert r["d"] == r["ref_d"], (r["d"], r["ref_d"])


def test_count_pass_in_place(hiplib, oracle):
    """count_pass over the stored N plane of every site: 147 457 groups, cut by the 2^16-group bound alone (TRACS_KSPLIT=1)"""
    _count_pass(True)


def test_count_pass_repacked(hiplib, oracle):
    """count_pass over the re-packed N plane of the counted sites (95 % of them: still beyond 2^16 groups)"""
    _count_pass(False)


@pytest.mark.parametrize("kind", ["consensus", "general"])
def test_valu_control(kind, hiplib, oracle):
    """TRACS_MFMA=0: the integer VALU kernel on the same input -- a failure above that this one does not share is the accumulators'"""
    r = _child(kind, {"TRACS_MFMA": "0"})
    assert r["encoding"] == kind and r["kernel"] == "valu" and r["classes"] is None
    assert r["d"] == r["ref_d"] and r["nn"] == r["ref_nn"]
