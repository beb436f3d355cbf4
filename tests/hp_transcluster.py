"""transcluster's log P(direct) and E(K) evaluated from the series' definition in high precision (mpmath).

TEST INFRASTRUCTURE ONLY: tests/golden/make_golden.py (hp-transcluster) writes tests/golden/transcluster_hp_golden.json with it,
and tests/test_transcluster_hp.py recomputes a sample of that fixture.  The GPU tests read the fixture only.

For one key (N SNPs, delta years, rates lamb and beta, threshold thr), with delta taken exactly as the double the kernels see:

    P_N = sum_{i<=N} (lamb delta)^i / i!          S_M = sum_{j<=M} (delta (lamb + beta))^j / j!
    p0  = ln[ lamb^(N+1) e^(-delta beta) S_N / ((lamb + beta)^(N+1) P_N) ]                      (delta > 0)
    p0  = (N + 1) ln(lamb / (lamb + beta))                                                       (delta = 0, the closed form)

E(K) is the reference's loop over k = 1, 2, ..: its term  l_k = k b_k S_{N+k} e^(-delta (lamb + beta))  with
b_k = lamb^(N+1) beta^k C(N+k, k) e^(delta lamb) / ((lamb + beta)^(N+k+1) P_N), and the stopping sum's term e_k = k b_k
(delta = 0: S = P = 1, and e_k carries a second factor (lamb + beta)^-(N+k+1), as the reference's closed-form branch does).
The loop ends after the first k with  diff_k = upper - sum_{j<=k} e_j <= thr,  or after k = 9 999, where
upper = beta (N + 1) e^(delta lamb) / (lamb P_N) (= the sum of all e_k when delta > 0).  E(K) = sum_{k <= k_stop} l_k.

Overflow: where upper exceeds the largest double it is +inf in any double evaluation, and so is diff_k until the stopping
sum itself exceeds the largest double; from there on diff_k = inf - inf is NaN and the loop's test (diff > thr) ends it.  So with
upper beyond the largest double the loop stops after the first k whose stopping sum exceeds the largest double, or at 9 999.

Class of a key: with margin = 1e-10 upper, k_lo (k_hi) is the first k with diff_k <= thr + margin (<= thr - margin), both
capped at 9 999 (upper beyond the largest double D: the first k with a stopping sum >= D (1 - 1e-10) (>= D (1 + 1e-10))).  A double evaluation of the loop stops within [k_lo, k_hi].  k_lo == k_hi: 'saturated' when that is 9 999,
'determined' otherwise; k_lo < k_hi: 'ill' (the stop is decided by rounding).
"""
import sys

from mpmath import mp, mpf

DPS = 40
K_CAP = 10000                  # the loop runs while k < 10 000
MARGIN = 1e-10
YEAR_S = 31556952.0
DBL_MAX = sys.float_info.max


def day_delta(gap):
    """delta in years of a whole-day gap, as the dense kernels compute it"""
    return gap * 86400.0 / YEAR_S


def _ln(x):
    return float(mp.log(x)) if x > 0 else float("-inf")


def evaluate(N, delta, lamb, beta, thr):
    """-> dict(p0, ln_eK, k_stop, cls, k_lo, k_hi, ln_e_lo, ln_e_hi, ln_upper) for one key (all logs natural, as doubles)"""
    N = int(N)
    with mp.workdps(DPS):
        d, L, B, T = mpf(float(delta)), mpf(float(lamb)), mpf(float(beta)), mpf(float(thr))
        lb = L + B
        if d > 0:
            x, y = L * d, d * lb
            P = t = mpf(1)
            for i in range(1, N + 1):
                t = t * x / i
                P += t
            S = tS = mpf(1)
            for j in range(1, N + 1):
                tS = tS * y / j
                S += tS
            p0 = mp.log(L ** (N + 1) * mp.exp(-d * B) * S / (lb ** (N + 1) * P))
            upper = B * (N + 1) * mp.exp(d * L) / (L * P)
            scale_F = mp.exp(-y)
            b = L ** (N + 1) * B * (N + 1) * mp.exp(d * L) / (lb ** (N + 2) * P)    # b_1
            e_extra = mpf(1)
        else:
            y = mpf(0)
            S = tS = mpf(1)
            p0 = (N + 1) * mp.log(L / lb)
            upper = B * (N + 1) / L
            scale_F = mpf(1)
            b = L ** (N + 1) * B * (N + 1) / lb ** (N + 2)
            e_extra = 1 / lb ** (N + 2)                                            # (lamb + beta)^-(N+k+1) at k = 1
        DMAX = mpf(DBL_MAX)
        infinite = upper > DMAX
        margin = MARGIN * upper
        E = Esum = mpf(0)
        k_lo = k_hi = k_stop = None
        e_at = {}
        for k in range(1, K_CAP):
            M = N + k
            if d > 0:
                tS = tS * y / M
                S += tS
            E += k * b * S * scale_F
            Esum += k * b * e_extra
            if not infinite:
                diff = upper - Esum
                lo, stop, hi = diff <= T + margin, diff <= T, diff <= T - margin
            else:
                lo, stop, hi = Esum >= DMAX * (1 - MARGIN), Esum > DMAX, Esum >= DMAX * (1 + MARGIN)
            if k_lo is None and lo:
                k_lo = k
            if k_stop is None and stop:
                k_stop = k
            if k_hi is None and hi:
                k_hi = k
            if k in (k_lo, k_stop, k_hi):
                e_at[k] = +E
            if k_hi is not None:
                break
            b = b * B * (M + 1) / ((k + 1) * lb)
            if d <= 0:
                e_extra = e_extra / lb
        last = K_CAP - 1
        if k_hi is None:
            e_at[last] = +E
        k_lo = last if k_lo is None else k_lo
        k_stop = last if k_stop is None else k_stop
        k_hi = last if k_hi is None else k_hi
        cls = "ill" if k_lo != k_hi else ("saturated" if k_stop == last else "determined")
        return {"p0": float(p0), "ln_eK": _ln(e_at[k_stop]), "k_stop": k_stop, "cls": cls, "k_lo": k_lo, "k_hi": k_hi,
                "ln_e_lo": _ln(e_at[k_lo]), "ln_e_hi": _ln(e_at[k_hi]), "ln_upper": float(mp.log(upper))}
