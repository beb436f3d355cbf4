"""The branches of the dense call's host driver (csrc/pairsnp.hip) that no other test names: the exits before any
pair kernel (no sites, no tile), the stage without a dense site, and the two-pass thresholded stage on site classes, whose counting
pass gets the live tiles only.  The driver's switches are read per process: every case is a child process, checked exactly
against the oracle on the same sequences."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = r'''
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from oracle import oracle as O
from tracs_amd import device as dev, synth, _lib
SENT = 0x55555555
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)

def filled(n):
    return torch.full((n, n), SENT, dtype=torch.int32, device="cuda"), torch.full((n, n), SENT, dtype=torch.int32, device="cuda")

def armed():
    """an event the next dense call has to record, and one recorded (and reached) before it"""
    before, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e.record(); before.record(); torch.cuda.synchronize()
    dev.notify_distances(e)
    return before, e

def recorded_by_the_call(before, e):
    torch.cuda.synchronize()
    assert e.query()
    assert before.elapsed_time(e) >= 0.0, before.elapsed_time(e)       # recorded again, behind `before`

def check(aln, seqs, thr=None):
    """d and nn of one dense call against the oracle: every pair, or the pairs within thr (the others > thr or negative)"""
    n = seqs.shape[0]
    er, ec, ed, enn = O.pairsnp_arrays(seqs, n_threads=8)
    ri, ci = er.astype(np.int64), ec.astype(np.int64)
    d = torch.zeros((n, n), dtype=torch.int32, device="cuda"); nn = torch.zeros_like(d)
    dev.pairsnp_dense(aln, d, nn, dist_threshold=thr)
    keep = np.ones(len(ed), dtype=bool) if thr is None else ed <= thr
    dh, nh = d.cpu().numpy(), nn.cpu().numpy()
    assert np.array_equal(dh[ri[keep], ci[keep]], ed[keep].astype(np.int32)), ("d", thr)
    assert np.array_equal(nh[ri[keep], ci[keep]], enn[keep].astype(np.int32)), ("nn", thr)
    far = dh[ri[~keep], ci[~keep]].astype(np.int64)
    assert ((far > (thr or 0)) | (far < 0)).all()
'''

NO_SITES = HEAD + r'''
n = 5
aln = dev.Alignment(n, 0)                                   # never packed
er, ec, ed, enn = O.pairsnp_arrays(np.zeros((n, 0), dtype=np.uint8))
assert not ed.any() and not enn.any()
d, nn = filled(n)
before, e = armed()
dev.pairsnp_dense(aln, d, nn)
recorded_by_the_call(before, e)
up = np.triu(np.ones((n, n), dtype=bool), 1)
for m in (d.cpu().numpy(), nn.cpu().numpy()):
    assert (m[up] == 0).all() and (m[~up] == SENT).all()
aln.close()
'''

NO_TILE = HEAD + r'''
import ctypes as C
n, L = 70, 777
seqs = synth.alignment(n, L, seed=n + L, mu_lineage=2e-3, mu_sample=3e-4, n_lineages=5, p_n=0.02, p_partial=0.02, p_other=0.001)
aln = dev.Alignment(n, L)
aln.pack(seqs)
lib = _lib.load()
lib.tracs_debug_pair_timing(1)
def last_ms():
    out = (C.c_float * 4)()
    assert lib.tracs_debug_pair_ms_mean(1, out) == 0
    return [float(x) for x in out]
check(aln, seqs)
torch.cuda.synchronize()
ms = last_ms()
d, nn = filled(n)
before, e = armed()
dev.pairsnp_dense(aln, d, nn, row_begin=n - 1, row_end=n)   # the last row has no cell right of the diagonal: no tile
recorded_by_the_call(before, e)
assert (d.cpu().numpy() == SENT).all() and (nn.cpu().numpy() == SENT).all()
assert last_ms() == ms                                       # the call counter did not move: still the call before
lib.tracs_debug_pair_timing(0)
aln.close()
'''

# every sample a copy of one ancestor with substitutions at sites of its own: each variable site lists one sample and goes to the
# minority lists, nothing is left for the pair kernel.  Sample 0 is the ancestor itself and never N at those sites: a site's reference
# base is the base of its lowest-index sample that is not N, and where that sample is the one that differs every other sample is
# listed and the site is dense.  (No partial code either: its site would be dense.  TRACS_FORCE_GENERAL keeps the general encoding
# all the same: the route without a pair kernel that reports "mfma-general".)
NO_DENSE_SITE = HEAD + r'''
n, L = 70, 3000
rng = np.random.default_rng(3)
anc = rng.integers(0, 4, L)
idx = np.tile(anc, (n, 1))
own = rng.permutation(L)[:n * 20].reshape(n, 20)            # 20 private sites per sample
for s in range(1, n):
    idx[s, own[s]] = (anc[own[s]] + rng.integers(1, 4, 20)) %% 4
seqs = BASES[idx]
isn = rng.random((n, L)) < 0.02
isn[0, own.ravel()] = False
seqs[isn] = ord("N")
aln = dev.Alignment(n, L)
aln.pack(seqs)
check(aln, seqs)
print("CLASSES", aln.site_classes, "KERNEL", aln.kernel, "ENC", aln.encoding)
assert aln.site_classes is not None and aln.site_classes[0] == 0, aln.site_classes      # no dense site
assert aln.kernel == %(kernel)r, aln.kernel
ed = O.pairsnp_arrays(seqs, n_threads=8)[2]
check(aln, seqs, thr=int(np.percentile(ed, 30)))
assert aln.site_classes[0] == 0 and aln.kernel == %(kernel)r
aln.close()
'''

# four lineages of 32 samples and a far fifth of three (the last three samples): the lineages' mutations are shared by many samples
# -- dense sites, >= 128 groups of them -- and with the threshold at the largest distance inside a lineage the 128 x 128 block
# rows 0..127 x columns 128..130 is dead, the block of the last three samples entirely alive, the large one mixed
TWO_PASS = HEAD + r'''
n, L = 131, 48000
rng = np.random.default_rng(11)
anc = rng.integers(0, 4, L)
lin = np.tile(anc, (5, 1))
for k in range(5):
    m = rng.random(L) < 0.15
    lin[k, m] = (lin[k, m] + rng.integers(1, 4, int(m.sum()))) %% 4
of = np.concatenate([np.repeat(np.arange(4), 32), np.full(3, 4)])
idx = lin[of]
m = rng.random((n, L)) < 3e-4
idx[m] = (idx[m] + rng.integers(1, 4, int(m.sum()))) %% 4
seqs = BASES[idx]
seqs[rng.random((n, L)) < 0.02] = ord("N")
er, ec, ed, enn = O.pairsnp_arrays(seqs, n_threads=8)
same = of[er.astype(np.int64)] == of[ec.astype(np.int64)]
thr = int(ed[same].max())
beyond = ed > thr
blk = (er // 128) * 2 + ec // 128                            # 128 x 128 blocks of the pair matrix: 0, 1, 3
assert any(beyond[blk == b].all() for b in (0, 1, 3)) and any(not beyond[blk == b].any() for b in (0, 1, 3))
assert beyond.any() and not beyond.all()
aln = dev.Alignment(n, L)
aln.pack(seqs)
check(aln, seqs, thr=thr)
print("CLASSES", aln.site_classes, "KERNEL", aln.kernel, "COUNT", aln.count_source)
assert aln.site_classes is not None and aln.site_classes[0] >= 128 * 128, aln.site_classes
check(aln, seqs)
aln.close()
'''

CASES = [
    ("no-sites", NO_SITES, {}, {}),
    ("no-tile", NO_TILE, {}, {}),
    ("no-dense-site", NO_DENSE_SITE, {"TRACS_SITE_CLASSES": "1", "TRACS_FORCE_GENERAL": "1"}, {"kernel": "mfma-general"}),
    ("no-dense-site-consensus", NO_DENSE_SITE, {"TRACS_SITE_CLASSES": "1"}, {"kernel": "mfma"}),
    ("two-pass", TWO_PASS, {"TRACS_SITE_CLASSES": "1"}, {}),
    ("two-pass-prefix-2", TWO_PASS, {"TRACS_SITE_CLASSES": "1", "TRACS_THR_PREFIX": "2"}, {}),
    ("one-pass", TWO_PASS, {"TRACS_SITE_CLASSES": "1", "TRACS_THR_ONE_PASS": "1"}, {}),
    ("two-pass-in-place-ksplit-3", TWO_PASS, {"TRACS_SITE_CLASSES": "1", "TRACS_COUNT_IN_PLACE": "1", "TRACS_KSPLIT": "3"}, {}),
]


@pytest.mark.parametrize("script,env,args", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_dense_driver_branch(hiplib, oracle, script, env, args):
    out = subprocess.run([sys.executable, "-c", script % dict(args, root=ROOT)], capture_output=True, text=True,
                         env=dict(os.environ, **env), timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
