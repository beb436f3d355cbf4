"""The oracle against oracle/_ref (the reference's transcluster.hpp / dmultinomial.hpp compiled in place): against its outputs
stored under tests/golden/ (tests/golden/make_golden.py oracle-vs-ref) everywhere, and against the live build as well where
oracle/_ref is present.  Runs in a SUBPROCESS: the reference is built with -ffast-math, and loading such a library switches the
whole process to flush-to-zero arithmetic."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "oracle_vs_ref_golden.npz")

SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, %r)
from oracle import oracle as O
G = np.load(%r)
R = O.ref_module()
sources = ["stored"] + (["live"] if R is not None else [])
bad = 0
for src in sources:
    for t in range(3):
        lamb, beta = G["lamb_beta_%%d" %% t].tolist()
        N, days = G["N_%%d" %% t], G["days_%%d" %% t]
        delta = days * 86400.0 / 31556952.0
        p0, ek = O.trans_dist(N, delta, lamb, beta, 0.01)
        if src == "stored":
            rp0, rek = G["p0_%%d" %% t], G["ek_%%d" %% t]
        else:
            rp0, rek = R.ref_trans_dist(N.tolist(), delta.tolist(), lamb, beta, 0.01)
        assert np.allclose(p0, rp0, rtol=1e-12, atol=0), src
        for i in range(400):
            cls = O.ek_conditioning(int(N[i]), float(delta[i]), lamb, beta, 0.01)[0]
            if cls == "well":
                assert abs(ek[i] - rek[i]) <= 1e-9 * abs(rek[i]), (src, lamb, N[i], days[i], ek[i], rek[i])
            elif abs(ek[i] - rek[i]) > 1e-9 * abs(rek[i]):
                bad += 1
    counts = G["counts"]
    for keep in (False, True):
        a = O.calculate_posteriors(counts, [3.0, 0.2, 9.0, 0.7], keep, 0.04)
        if src == "stored":
            b = G["posteriors_keep_%%d" %% keep]
        else:
            b = np.asarray(R.ref_calculate_posteriors(counts, [3.0, 0.2, 9.0, 0.7], keep, 0.04))
        assert np.max(np.abs(a - b)) <= 4e-16, src
print("OK", "+".join(sources), "ill/saturated disagreements:", bad)
'''


def test_oracle_matches_reference_build():
    out = subprocess.run([sys.executable, "-c", SCRIPT % (ROOT, GOLDEN)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
