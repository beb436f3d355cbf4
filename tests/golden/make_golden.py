#!/usr/bin/env python3
"""Generate the committed golden fixtures under tests/golden/ (run in the build container only).

Sources of truth, in order of authority:
  * oracle/_ref  -- the reference's own src/transcluster.hpp + src/dmultinomial.hpp + src/kseq.h compiled
    from where they lie under /root/reference with setup.py's flags (oracle/Makefile);
  * the reference's Python drivers imported from /root/reference (tracs/transcluster.py, tracs/cluster.py,
    tracs/distance.py, tracs/dirichlet_multinomial.py) with a stub `TRACS` module whose trans_dist /
    calculate_posteriors / lprob_k_given_N are oracle/_ref and whose pairsnp is the reference's own
    src/pairsnp.hpp, compiled in place over oracle/boost_standin (oracle/_ref/_tracs_ref_pairsnp: Boost is
    absent here, so the bitset and the binomial CDF it includes are our stand-ins; everything else --
    load_seqs, the pair loop, range_count, filter_recomb's control flow -- is the reference's).
    `pairsnp-ref` records that module's outputs (pairsnp_ref_golden.npz); pairsnp_unpinned.json holds the
    oracle's values, asserted equal to the reference's and to an independent numpy brute force.
Only DATA is written (inputs + expected outputs); no reference source text is stored.
"""
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"

from oracle import oracle as O  # noqa: E402
from tracs_amd import synth  # noqa: E402

R = O.ref_module()
assert R is not None or sys.argv[1:] in (["hp-transcluster"], ["hp-filter"], ["hp-dirichlet"]), "oracle/_ref is not built (make -C oracle)"


def jdump(name, obj):
    with open(os.path.join(HERE, name), "w") as fh:
        json.dump(obj, fh, indent=1)
    print("wrote", name)


# ---------------------------------------------------------------------------------------
def transcluster():
    rng = np.random.default_rng(20241022)
    out = {"known_answers": {
        # /root/reference/tests/test_llk.py:21-29
        "lprob_k_given_N": {"args": [7, 4, 0.16963, 3, 52], "lgamma_len": 20,
                            "expect": [-17.9565184209608, 12.0861694243766], "atol": 1e-6},
        # /root/reference/tests/test_trans_distance.py:29-42 (1-day gap; SNP 0 and 2; CLI defaults)
        "trans_distance": {"snp": [0, 2], "delta": [0.002737907006988508] * 2, "lamb": 1e-3 * 29903, "beta": 73.0,
                           "precision": 0.01, "p_direct": [0.23794988406662973, 0.024467137572328577],
                           "expected_k": [2.6335200453700187, 7.315670110063259], "atol": 1e-6}}}
    grids = []
    for lamb, beta, thr in ((1e-3 * 29903, 73.0, 0.01), (5.3, 6.0, 0.01), (3.0, 52.0, 0.01), (5.3, 6.0, 1e-4),
                            (20.0, 2.0, 0.05)):
        N = np.concatenate([np.arange(0, 12), rng.integers(0, 120, 60)]).astype(int)
        days = np.concatenate([np.zeros(6, int), rng.integers(1, 700, N.size - 6)])
        delta = days.astype(np.float64) * 86400.0 / 31556952.0
        p0, ek = R.ref_trans_dist(N.tolist(), delta.tolist(), lamb, beta, thr)
        cls = [O.ek_conditioning(int(n), float(d), lamb, beta, thr)[0] for n, d in zip(N, delta)]
        grids.append({"lamb": lamb, "beta": beta, "thr": thr, "N": N.tolist(), "days": days.tolist(),
                      "delta": delta.tolist(), "p0": list(p0), "eK": list(ek), "conditioning": cls})
    out["trans_dist"] = grids
    lg = [float(x) for x in __import__("scipy.special", fromlist=["gammaln"]).gammaln(np.arange(300))]
    rows = []
    for _ in range(60):
        N, k = int(rng.integers(0, 120)), int(rng.integers(0, 120))
        delta = float(rng.choice([0.0, 0.0027379070069885, 0.05, 0.4, 1.7]))
        lamb, beta = (5.3, 6.0) if rng.random() < 0.5 else (29.903, 73.0)
        a = R.ref_lprob_k_given_N(N, k, delta, lamb, beta, lg)
        b = R.ref_lprob_k_given_N_2(N, k, delta, lamb, beta)
        rows.append({"N": N, "k": k, "delta": delta, "lamb": lamb, "beta": beta, "lprob_k_given_N": list(a),
                     "lprob_k_given_N_2": list(b)})
    out["lprob"] = {"lgamma_len": 300, "rows": rows}
    jdump("transcluster_golden.json", out)


def transcluster_large_n():
    """Keys with hundreds to thousands of SNPs (the bench workload's range: mean d ~ 1 000) through oracle/_ref: these take the
    device's wave-per-key kernel from their first term (csrc/transcluster.hip, TC_WAVE_PREFIX_MIN).  A file of its own so the
    older fixtures stay byte-identical."""
    rng = np.random.default_rng(20261002)
    grids = []
    for lamb, beta, thr in ((1e-3 * 29903, 73.0, 0.01), (5.3, 6.0, 0.01)):
        N = np.concatenate([[128, 129, 191, 192, 193, 1000], rng.integers(128, 1600, 40)]).astype(int)
        days = np.concatenate([[1, 30, 365, 700, 2, 3], rng.integers(1, 700, N.size - 6)])
        delta = days.astype(np.float64) * 86400.0 / 31556952.0
        p0, ek = R.ref_trans_dist(N.tolist(), delta.tolist(), lamb, beta, thr)
        cls = [O.ek_conditioning(int(n), float(d), lamb, beta, thr)[0] for n, d in zip(N, delta)]
        grids.append({"lamb": lamb, "beta": beta, "thr": thr, "N": N.tolist(), "days": days.tolist(),
                      "delta": delta.tolist(), "p0": list(p0), "eK": list(ek), "conditioning": cls})
    jdump("transcluster_golden_large_n.json", {"trans_dist": grids})


def transcluster_outbreak():
    """4 000 outbreak-scale keys at the CLI defaults (N <= 80 SNPs, 1..730 days, lamb = 29.903, beta = 73, precision 0.01) -- the
    regime TRACS is used in, where a few percent of the keys have their E(K) stopping point decided by rounding ('ill').  Three
    columns: the reference as shipped (oracle/_ref: setup.py's -ffast-math), the SAME source compiled IEEE-strict
    (oracle/_ref/_tracs_ref_strict), and the oracle's conditioning class.  Each build runs in its own child process (loading the
    fast-math library switches a process to flush-to-zero)."""
    rng = np.random.default_rng(20261003)
    n_keys = 4000
    N = rng.integers(0, 81, n_keys)
    days = rng.integers(1, 731, n_keys)
    lamb, beta, thr = 1e-3 * 29903, 73.0, 0.01
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "keys.npz")
        np.savez(f, N=N, days=days)
        code = ("import sys, json, numpy as np\n"
                "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
                "import importlib; M = importlib.import_module(sys.argv[2])\n"
                "z = np.load(sys.argv[1]); N = z['N'].tolist(); d = (z['days'].astype(np.float64) * 86400.0 / 31556952.0).tolist()\n"
                "p0, ek = M.ref_trans_dist(N, d, %r, %r, %r)\n"
                "out = {'p0': list(p0), 'eK': list(ek)}\n"
                "if sys.argv[2].endswith('strict'):\n"
                "    from oracle import oracle as O\n"
                "    out['cls'] = [O.ek_conditioning(int(n), float(x), %r, %r, %r)[0] for n, x in zip(N, d)]\n"
                "print(json.dumps(out))\n" % (ROOT, os.path.join(ROOT, "oracle", "_ref"), lamb, beta, thr, lamb, beta, thr))
        res = {}
        for mod in ("_tracs_ref", "_tracs_ref_strict"):
            o = subprocess.run([sys.executable, "-c", code, f, mod], capture_output=True, text=True, timeout=7200)
            assert o.returncode == 0, o.stderr[-2000:]
            res[mod] = json.loads(o.stdout.strip().splitlines()[-1])
    fast, strict = res["_tracs_ref"], res["_tracs_ref_strict"]

    def clean(v):
        return [x if np.isfinite(x) else None for x in v]
    jdump("transcluster_outbreak_golden.json",
          {"lamb": lamb, "beta": beta, "thr": thr, "N": N.tolist(), "days": days.tolist(),
           "p0": fast["p0"], "eK": clean(fast["eK"]), "eK_strict_build": clean(strict["eK"]), "conditioning": strict["cls"],
           "note": "eK: the reference as shipped (-ffast-math); eK_strict_build: the same headers compiled without it; null = inf / nan"})


def posteriors():
    counts = synth.allele_counts(4000, seed=11, depth=20, p_two=0.08).astype(np.float64)
    counts[:40] = 0
    counts[40:80] = 5
    counts[80:120, 2] = counts[80:120, 0]
    counts[120:160, 3] = counts[120:160, 1]
    counts[160:170] = [[3, 3, 1, 1]] * 10
    cases = []
    for alphas in ([20.8156311152126, 4.38181182238621, 0.889048781117318, 0.1], [0.5, 12.0, 0.05, 3.0], [0, 0, 0, 1.0]):
        for keep in (False, True):
            for thr in (0.0, 0.01, 0.1):
                post = R.ref_calculate_posteriors(counts, list(alphas), keep, thr)
                cases.append({"alphas": alphas, "keep": keep, "threshold": thr, "posterior": np.asarray(post)})
    np.savez_compressed(os.path.join(HERE, "posteriors_golden.npz"), counts=counts,
                        meta=json.dumps([{k: c[k] for k in ("alphas", "keep", "threshold")} for c in cases]),
                        **{"post_%d" % i: c["posterior"] for i, c in enumerate(cases)})
    print("wrote posteriors_golden.npz")


KSEQ_CASES = {
    "plain": ">s1\nACGT\n>s2 desc text\nAC\nGT\n",
    "wrapped_crlf": ">a\r\nAC\r\nGT\r\n>b\r\nTTGA\r\n",
    "leading_junk": "junk line\n\n>x\nACGTN\n",
    "no_trailing_newline": ">x\nACGT\n>y\nAC-T",
    "lower_and_iupac": ">m\nacgtRYKMswbdhvn-?.*\n",
    "fastq": "@r1 c\nACGT\n+\nIIII\n@r2\nTTGA\n+r2\n!!!!\n",
    "fastq_short_qual": "@r1\nACGT\n+\nII\n",
    "gt_inside_sequence": ">a\nAC>b\nGT\n",
    "tabs_and_spaces": ">name\twith tab\nA C\tG T\n",
    "empty_name": ">\nACGT\n",
    "empty_file": "",
    "header_only": ">lonely",
    "at_header_fasta_body": "@odd\nACGT\n>next\nTTTT\n",
    "blank_lines": ">a\n\nAC\n\nGT\n\n>b\nAAAA\n",
}


def kseq():
    dump = O.kseq_dump_path()
    assert dump
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for name, text in KSEQ_CASES.items():
            p = os.path.join(td, name)
            with open(p, "wb") as fh:
                fh.write(text.encode("latin-1"))
            pr = subprocess.run([dump, p], capture_output=True)
            if pr.returncode != 0:          # the reference's reader itself crashes (e.g. a header with no sequence bytes
                out[name] = {"text": text, "crash": True}      # dereferences a NULL kstring): behaviour undefined, not a fixture
                continue
            res = pr.stdout.decode("latin-1")
            lines = res.split("\n")
            rc = int([ln for ln in lines if ln.startswith("#rc=")][0][4:])
            recs = [ln.split("\t") for ln in lines if ln and not ln.startswith("#rc=")]
            out[name] = {"text": text, "rc": rc, "records": [[r[0], r[1] if len(r) > 1 else ""] for r in recs]}
    jdump("kseq_golden.json", out)


def oracle_vs_ref():
    """The inputs of tests/test_oracle_vs_ref.py and oracle/_ref's outputs for them, so that the test also runs where oracle/_ref
    cannot be built: trans_dist on 400 keys for each of three (lamb, beta), calculate_posteriors on 2 000 count rows."""
    rng = np.random.default_rng(5)
    out = {}
    for t, (lamb, beta) in enumerate(((5.3, 6.0), (29.903, 73.0), (3.0, 52.0))):
        N = rng.integers(0, 90, 400); days = rng.integers(0, 300, 400); days[:20] = 0
        delta = days * 86400.0 / 31556952.0
        rp0, rek = R.ref_trans_dist(N.tolist(), delta.tolist(), lamb, beta, 0.01)
        out.update({"lamb_beta_%d" % t: np.array([lamb, beta]), "N_%d" % t: N.astype(np.int64), "days_%d" % t: days.astype(np.int64),
                    "p0_%d" % t: np.asarray(rp0, np.float64), "ek_%d" % t: np.asarray(rek, np.float64)})
    counts = rng.poisson(6, (2000, 4)).astype(float); counts[:30] = 0; counts[30:60] = 4
    out["counts"] = counts
    for keep in (False, True):
        out["posteriors_keep_%d" % keep] = np.asarray(R.ref_calculate_posteriors(counts, [3.0, 0.2, 9.0, 0.7], keep, 0.04), np.float64)
    np.savez_compressed(os.path.join(HERE, "oracle_vs_ref_golden.npz"), **out)
    print("wrote oracle_vs_ref_golden.npz")


def _ref_pairsnp_both(fastas, dist, filt):
    """ref_pairsnp through both builds of the reference's source (setup.py's flags, IEEE-strict): equal, or nothing is recorded"""
    a = O.ref_pairsnp_module().ref_pairsnp(fastas, 1, int(dist), bool(filt))
    b = O.ref_pairsnp_module(strict=True).ref_pairsnp(fastas, 1, int(dist), bool(filt))
    assert a == b, ("the fast-math and the strict build of the reference disagree", fastas, dist, filt)
    return a


def pairsnp_unpinned():
    sys.path.insert(0, os.path.dirname(HERE))
    import pairsnp_ref_cases as PC
    cases = {}
    specs = {"iupac_small": dict(n=7, L=61, seed=3, mu_lineage=0.05, mu_sample=0.03, p_n=0.05, p_partial=0.1, p_lower=0.2, p_other=0.05),
             "tail_129": dict(n=12, L=129, seed=4, mu_lineage=0.02, mu_sample=0.02, p_n=0.02, p_partial=0.02),
             "consensus_300": dict(n=20, L=300, seed=5, mu_lineage=0.01, mu_sample=0.01, p_n=0.03)}
    for name, kw in specs.items():
        seqs = synth.alignment(**kw)
        for mode, n0, dist in (("all", None, 2147483647), ("thr", None, 4), ("twofile", kw["n"] // 3, 2147483647)):
            a = O.pairsnp_arrays(seqs, n0=n0, dist=dist)
            b = O.brute_pairsnp(seqs, n0=n0, dist=dist)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), "oracle != brute force"
            with tempfile.TemporaryDirectory() as td:           # and the reference's own pair loop on the same samples
                fas = PC.write_fastas(dict(name=name + mode, n0=n0, width=0, crlf=False, gz=False), seqs, td)
                ref = _ref_pairsnp_both(fas, dist, False)
            assert all(np.array_equal(x, np.asarray(y, np.uint64)) for x, y in zip(a, (ref[0], ref[1], ref[2], ref[5]))), "oracle != reference"
            cases["%s/%s" % (name, mode)] = {"seqs": [row.tobytes().decode("ascii") for row in seqs], "n0": n0, "dist": dist,
                                             "rows": a[0].tolist(), "cols": a[1].tolist(), "d": a[2].tolist(),
                                             "nn": a[3].tolist()}
    jdump("pairsnp_unpinned.json", {"status": "formerly PARITY UNPINNED, now pinned: produced by oracle/tracs_oracle.c, and asserted by the generator "
                                              "to equal the reference's own src/pairsnp.hpp compiled in place over oracle/boost_standin "
                                              "(oracle/_ref/_tracs_ref_pairsnp, both builds) and oracle.brute_pairsnp",
                                    "cases": cases})

# ---------------------------------------------------------------------------------------
# The reference's own pair loop and recombination filter (oracle/_ref/_tracs_ref_pairsnp: src/pairsnp.hpp compiled in place over
# oracle/boost_standin), recorded with its inputs: tests/golden/pairsnp_ref_golden.npz (layout: tests/pairsnp_ref_cases.py).
_SUBST = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGTacgt", b"CGTAcgta"):
    _SUBST[_a] = _b


def _plant(seqs, samples, a, b, share, seed):
    """an import: the same substitutions on `share` of the sites [a, b) in every listed sample (N and partial codes stay)"""
    hit = a + np.nonzero(np.random.default_rng(seed).random(b - a) < share)[0]
    for s in samples:
        row = seqs[s, hit]
        seqs[s, hit] = np.where(_SUBST[row] != 0, _SUBST[row], row)


def _pairsnp_ref_alignments():
    alns = {}
    with open(os.path.join(HERE, "pairsnp_unpinned.json")) as fh:
        unp = json.load(fh)["cases"]
    for name in ("iupac_small", "tail_129", "consensus_300"):
        alns[name] = np.array([np.frombuffer(r.encode("ascii"), np.uint8) for r in unp[name + "/all"]["seqs"]])
    # every printable byte but the three kseq reads as the start of a record or of a quality line, against each base: the switch's
    # default branch and toupper
    by = np.array([b for b in range(33, 127) if b not in b">+@"], np.uint8)
    rng = np.random.default_rng(11)
    rows = [np.tile(by, 4), np.repeat(np.frombuffer(b"ACGT", np.uint8), len(by)), np.tile(by[::-1], 4), np.tile(np.roll(by, 7), 4),
            np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 4 * len(by))]]
    swap = rows[0].copy()
    up, lo = (swap >= 65) & (swap <= 90), (swap >= 97) & (swap <= 122)
    swap[up] += 32
    swap[lo] -= 32
    alns["bytes"] = np.array(rows + [swap])
    for L in (1, 63, 64, 65, 127, 128, 129):
        alns["len_%d" % L] = synth.alignment(9, L, seed=100 + L, mu_lineage=0.1, mu_sample=0.1, n_lineages=2, p_n=0.05, p_partial=0.05,
                                             p_lower=0.1, p_other=0.02)
    alns["n70"] = synth.alignment(70, 4133, seed=70, mu_lineage=4e-3, mu_sample=2e-3, n_lineages=4, p_n=0.01, p_partial=0.003, p_lower=0.01)
    a = synth.alignment(130, 1000, seed=130, mu_lineage=1e-2, mu_sample=4e-3, n_lineages=6, p_n=0.01, p_partial=0.004, p_lower=0.01,
                        p_other=0.001)
    a[77] = a[12]                                              # two identical samples: dist = 0 emits a pair
    alns["n130"] = a
    same = synth.alignment(1, 200, seed=5, p_n=0.05, p_partial=0.05, p_lower=0.1)
    alns["identical"] = np.repeat(same, 5, axis=0)
    alns["all_differ"] = np.array([np.full(130, b, np.uint8) for b in b"ACGTa"])            # 'a' = 'A': one pair at d = 0 among them
    alln = synth.alignment(6, 100, seed=6, mu_sample=0.05, p_n=0.03)
    alln[2] = ord("N")
    alln[4] = np.frombuffer(b"n-?.*Xx", np.uint8)[np.arange(100) % 7]
    alns["all_n"] = alln
    return alns


def _filter_alignment(kind, seed):
    n, L = 8, 30000
    seqs = synth.alignment(n, L, seed=seed, mu_lineage=3e-3, mu_sample=1e-3, n_lineages=2, p_n=0.005, p_partial=0.001, p_lower=0.005)
    if kind == "dense_one":                                     # a dense stretch on one sample
        _plant(seqs, [3], 12000, 12300, 0.4, seed)
    elif kind == "lineage":                                     # the same stretch on every sample of one lineage
        _plant(seqs, [1, 3, 5, 7], 5000, 5400, 0.3, seed)
    else:                                                       # stretches that touch either end of the alignment
        _plant(seqs, [2], L - 250, L, 0.5, seed)
        _plant(seqs, [5], 0, 150, 0.6, seed + 1)
    return seqs


def _pair_windows(H, seqs, i, j):
    """-> (sorted SNP sites of the pair, [(count, length)] of its windows with count > 1)"""
    m = O._MASK[seqs]
    pos = np.nonzero((m[i] & m[j]) == 0)[0].astype(np.int64)
    L, d = seqs.shape[1], len(pos)
    if d <= 1:
        return pos, []
    _, _, wh = H.window(L, d)
    lo = np.searchsorted(pos, np.maximum(0, pos - wh), "left")
    hi = np.searchsorted(pos, np.minimum(L, pos + wh + 1), "left")
    count, length = hi - lo, pos[hi - 1] - pos[lo] + 1
    return pos, sorted({(int(k), int(n)) for k, n in zip(count, length) if k > 1})


def _hp_list_one(args):
    """one position list of filter_hp_golden.json through both builds of the reference and the definition"""
    import hp_filter as H
    L, d, pos = args
    a = O.ref_pairsnp_module().ref_filter_recomb_positions(L, pos.tolist())
    b = O.ref_pairsnp_module(strict=True).ref_filter_recomb_positions(L, pos.tolist())
    assert a == b, ("the two builds disagree", L, d)
    kept, _, ill, margin = H.filter_positions(pos, L)
    assert ill == 0 and margin > H.MARGIN, ("a window within the margin of its threshold", L, d, margin)
    assert kept == a, ("reference != definition", L, d, a, kept)
    return a, margin


def pairsnp_ref():
    import multiprocessing
    sys.path.insert(0, os.path.dirname(HERE))
    import hp_filter as H
    import pairsnp_ref_cases as PC
    RS = O.ref_pairsnp_module(strict=True)
    assert O.ref_pairsnp_module() is not None and RS is not None, "oracle/_ref/_tracs_ref_pairsnp is not built (make -C oracle)"
    alns = _pairsnp_ref_alignments()
    arrays, cases, filter_cases = {}, [], []
    plain = dict(n0=None, dist=PC.INT_MAX, filter=False, width=0, crlf=False, gz=False)

    def record(case, into):
        seqs = alns[case["aln"]]
        with tempfile.TemporaryDirectory() as td:
            out = _ref_pairsnp_both(PC.write_fastas(case, seqs, td), case["dist"], case["filter"])
        assert out[3] == PC.names_of(seqs.shape[0])
        for col, v in zip(PC.COLUMNS, (out[0], out[1], out[2], out[5], out[4])):
            arrays["%s/%s" % (case["name"], col)] = np.asarray(v, np.int64)
        into.append(case)
        return out

    for name in ("iupac_small", "tail_129", "consensus_300"):   # the alignments and modes of pairsnp_unpinned.json
        n = alns[name].shape[0]
        for mode, n0, dist in (("all", None, PC.INT_MAX), ("thr", None, 4), ("twofile", n // 3, PC.INT_MAX)):
            record(dict(plain, name="%s/%s" % (name, mode), aln=name, n0=n0, dist=dist), cases)
    for name in ["bytes"] + ["len_%d" % L for L in (1, 63, 64, 65, 127, 128, 129)] + ["n70", "identical", "all_differ", "all_n"]:
        record(dict(plain, name=name + "/all", aln=name), cases)
    full = record(dict(plain, name="n130/all", aln="n130"), cases)
    D = int(np.percentile(np.asarray(full[2]), 5))             # the exact d of some pair, so that d <= dist and d < dist differ
    assert D >= 2 and D in full[2] and 0 in full[2]
    for tag, dist in (("dist_minus1", -1), ("dist_0", 0), ("dist_d", D), ("dist_d_minus1", D - 1)):
        out = record(dict(plain, name="n130/" + tag, aln="n130", dist=dist), cases)
        assert len(out[2]) == int((np.asarray(full[2]) <= dist).sum())
    assert len(arrays["n130/dist_minus1/d"]) == 0 and len(arrays["n130/dist_0/d"]) >= 1
    assert len(arrays["n130/dist_d/d"]) > len(arrays["n130/dist_d_minus1/d"]) > 0
    for n0 in (1, 130 // 3, 129):
        record(dict(plain, name="n130/n0_%d" % n0, aln="n130", n0=n0), cases)
    record(dict(plain, name="n70/twofile_thr", aln="n70", n0=23, dist=int(np.median(arrays["n70/all/d"]))), cases)
    # the FASTA reader in front of the pair loop: wrapped lines, CRLF, gzip, and all three in two files
    record(dict(plain, name="tail_129/wrapped", aln="tail_129", width=60), cases)
    record(dict(plain, name="tail_129/crlf", aln="tail_129", crlf=True), cases)
    record(dict(plain, name="tail_129/gz", aln="tail_129", gz=True), cases)
    record(dict(plain, name="consensus_300/wrapped_crlf_gz_twofile", aln="consensus_300", n0=7, width=70, crlf=True, gz=True), cases)
    for a, b in (("tail_129/wrapped", "tail_129/all"), ("tail_129/crlf", "tail_129/all"), ("tail_129/gz", "tail_129/all")):
        assert all(np.array_equal(arrays["%s/%s" % (a, c)], arrays["%s/%s" % (b, c)]) for c in PC.COLUMNS)
    assert all(not arrays["%s/filt" % c["name"]].any() and len(arrays["%s/filt" % c["name"]]) == len(arrays["%s/d" % c["name"]])
               for c in cases)                                   # filter = False: a zero for every emitted pair

    # (b) planted imports through ref_pairsnp(filter = True); a seed with a window inside the margin is replaced, never tolerated
    cells, smallest, rejected = set(), 1.0, []
    for kind, first_seed in (("dense_one", 31), ("lineage", 41), ("end", 51)):
        for seed in range(first_seed, first_seed + 10):
            seqs = _filter_alignment(kind, seed)
            worst, kept_all, mine = 1.0, [], set()
            r, c, d, _ = O.brute_pairsnp(seqs)
            for i, j in zip(r.tolist(), c.tolist()):
                pos, win = _pair_windows(H, seqs, i, j)
                kept, _, ill, margin = H.filter_positions(pos, seqs.shape[1])
                worst = min(worst, margin if ill == 0 else 0.0)
                kept_all.append(kept)
                mine |= {(seqs.shape[1], len(pos), n, k) for k, n in win}
            if worst > H.MARGIN:
                break
            rejected.append((kind, seed, worst))
        else:
            raise AssertionError("no seed without an ill cell: " + kind)
        alns["filter_" + kind] = seqs
        out = record(dict(plain, name="filter_%s/filtered" % kind, aln="filter_" + kind, filter=True, width=80), filter_cases)
        assert out[4] == kept_all, ("reference != definition", kind)
        assert (np.asarray(out[4]) < np.asarray(out[2])).any() and (np.asarray(out[4]) <= np.asarray(out[2])).all()
        cells |= mine
        smallest = min(smallest, worst)
    off = record(dict(plain, name="filter_dense_one/unfiltered", aln="filter_dense_one", width=80), cases)
    assert off[4] == [0] * len(off[2]) and off[2] == arrays["filter_dense_one/filtered/d"].tolist()
    thr = record(dict(plain, name="filter_end/filtered_thr", aln="filter_end", filter=True,
                      dist=int(np.median(arrays["filter_end/filtered/d"]))), filter_cases)
    assert 0 < len(thr[2]) < len(arrays["filter_end/filtered/d"])

    # (a) every position list of filter_hp_golden.json through ref_filter_recomb_positions
    with open(os.path.join(HERE, "filter_hp_golden.json")) as fh:
        hp_cases = json.load(fh)["cases"]
    lists = PC.hp_lists(H, hp_cases)
    order = sorted(range(len(lists)), key=lambda t: -lists[t][1])          # the reference's filter is quadratic in d: longest first
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        res = pool.map(_hp_list_one, [lists[t] for t in order], chunksize=1)
    got = [None] * len(lists)
    for t, r in zip(order, res):
        got[t] = r
    arrays["hp/ref"] = np.asarray([g[0] for g in got], np.int64).reshape(len(hp_cases), 3)
    want = np.asarray([[c["expected"], c["probe"][1], c["probe"][2]] for c in hp_cases], np.int64)
    assert np.array_equal(arrays["hp/ref"], want), "reference != the 50-digit fixture"
    smallest = min([smallest] + [g[1] for g in got])

    # the stand-in CDF on the cells above and on n*, n* - 1 of every hp row: values of the strict build, and their error
    for c in hp_cases:
        cells |= {(c["L"], c["d"], n - e, k) for k, n in enumerate(c["row"], start=2) if n is not None for e in (0, 1)}
    cells = np.asarray(sorted(cells), np.int64)
    value = np.asarray([RS.ref_cached_binomial_cdf(int(n), float(d) / int(L), int(k)) for L, d, n, k in cells], np.float64)
    fast = O.ref_pairsnp_module()
    ratio = 0.0
    with H.mp.workdps(H.DPS):
        for (L, d, n, k), v in zip(cells.tolist(), value.tolist()):
            p, thr_, _ = H.window(L, d)
            for x in (v, fast.ref_cached_binomial_cdf(n, p, k)):
                ratio = max(ratio, float(abs(H.mpf(1.0 - x) - H.tail(n, k, p)) / H.mpf(thr_)))
    assert ratio <= H.MARGIN, ("the stand-in CDF misses the bound", ratio)
    arrays["cdf/cells"], arrays["cdf/value"] = cells, value
    for key, a in alns.items():
        arrays["aln/" + key] = a
    meta = {"about": "inputs, and what the reference's own src/pairsnp.hpp returned for them (oracle/_ref/_tracs_ref_pairsnp over "
                     "oracle/boost_standin; both builds equal); layout: tests/pairsnp_ref_cases.py",
            "cases": cases, "filter_cases": filter_cases, "hp_lists": len(lists), "margin": H.MARGIN, "digits": H.DPS, "dist_d": D,
            "measured": {"ill_cells": 0, "min_relative_margin": float("%.3g" % smallest), "cdf_cells": int(len(cells)),
                         "standin_max_error_over_threshold": float("%.3g" % ratio),
                         "rejected_seeds": [[k, s_, float("%.3g" % w)] for k, s_, w in rejected]}}
    PC.save(PC.FIXTURE, meta, arrays)
    print("wrote pairsnp_ref_golden.npz", os.path.getsize(PC.FIXTURE), "bytes;", len(cases), "+", len(filter_cases), "cases;",
          json.dumps(meta["measured"]))


def python_reference():
    """Golden outputs of the reference's Python drivers (imported from /root/reference)."""
    stub = types.ModuleType("TRACS")
    ref_pairsnp = O.ref_pairsnp_module().ref_pairsnp            # the reference's own pairsnp (oracle/_ref), no longer the oracle's
    stub.pairsnp = lambda fasta, n_threads, dist, filter: ref_pairsnp(fasta, 1, dist, filter)   # under the binding's argument names
    stub.trans_dist = R.ref_trans_dist
    stub.calculate_posteriors = R.ref_calculate_posteriors
    stub.lprob_k_given_N = R.ref_lprob_k_given_N
    sys.modules["TRACS"] = stub
    sys.modules.setdefault("pyfastx", types.ModuleType("pyfastx"))
    sys.path.insert(0, REF)
    import importlib
    ref_distance = importlib.import_module("tracs.distance")
    ref_cluster = importlib.import_module("tracs.cluster")
    ref_tc = importlib.import_module("tracs.transcluster")
    ref_dm = importlib.import_module("tracs.dirichlet_multinomial")
    out = {}
    with tempfile.TemporaryDirectory() as td:
        seqs = synth.alignment(14, 900, seed=21, mu_lineage=0.004, mu_sample=0.002, p_n=0.02, p_partial=0.01)
        names = ["iso%02d" % i for i in range(14)]
        msa = os.path.join(td, "refA_combined.fasta")
        synth.write_fasta(msa, seqs, names=names, width=80)
        iso, days = synth.dates(14, seed=21, span_days=120)
        meta = os.path.join(td, "dates.csv")
        with open(meta, "w") as fh:
            fh.write("sample,date\n")
            for nm, d in zip(names, iso):
                fh.write("%s,%s\n" % (nm, d))
        db = os.path.join(td, "db.fasta")
        synth.write_fasta(db, seqs[9:], names=names[9:])
        q = os.path.join(td, "query_combined.fasta.gz")
        synth.write_fasta(q, seqs[:9], names=names[:9], gz=True)
        runs = {"meta": ["--msa", msa, "--meta", meta], "nometa": ["--msa", msa],
                "meta_thr": ["--msa", msa, "--meta", meta, "-D", "6", "-K", "12", "--clock_rate", "5.3", "--trans_rate", "6.0"],
                "msadb": ["--msa", q, "--msa-db", db, "--meta", meta, "-D", "40"],
                "filter": ["--msa", msa, "--meta", meta, "--filter", "--clock_rate", "5.3", "--trans_rate", "6.0"],
                "filter_nometa": ["--msa", msa, "--filter", "-D", "30"]}
        csvs = {}
        for key, argv in runs.items():
            o = os.path.join(td, key + ".csv")
            sys.argv = [""] + argv + ["-o", o, "--loglevel", "ERROR"]
            ref_distance.main()
            csvs[key] = open(o).read().replace(td, "TMP")
        out["distance"] = {"seqs": [r.tobytes().decode() for r in seqs], "names": names, "dates": iso,
                           "runs": {k: {"argv": [a.replace(td, "TMP") for a in v], "csv": csvs[k]} for k, v in runs.items()}}
        # calculate_trans_prob (dates -> delta bits)
        rr, cc, dd, nm, _, _ = stub.pairsnp([msa], 1, 2147483647, False)
        dates = {n: (i, __import__("datetime").date.fromisoformat(i)) for n, i in zip(names, iso)}
        p0, ek, td_ = ref_tc.calculate_trans_prob([rr, cc, dd], sample_dates=dates, K=100, lamb=5.3, beta=6.0,
                                                  samplenames=nm, log=False, precision=0.01)
        out["calculate_trans_prob"] = {"rows": rr, "cols": cc, "d": dd, "days": days.tolist(), "lamb": 5.3, "beta": 6.0,
                                       "precision": 0.01, "p": list(map(float, p0)), "eK": list(map(float, ek)),
                                       "time_diff": list(map(float, td_))}
        # cluster: labels for each -D column
        clus = {}
        for col, thr in (("snp", 5), ("direct", 0.05), ("expectedK", 3.0), ("snp", 0)):
            o = os.path.join(td, "clu.csv")
            dist_csv = os.path.join(td, "meta.csv")
            ref_cluster.index_count.__dict__.pop("dict", None)
            ref_cluster.index_count.__dict__.pop("curr", None)
            sys.argv = ["", "-d", dist_csv, "-o", o, "-c", str(thr), "-D", col, "--loglevel", "ERROR"]
            ref_cluster.main()
            clus["%s_%s" % (col, thr)] = open(o).read()
        out["cluster"] = {"distance_csv": csvs["meta"], "runs": clus}
    # find_dirichlet_priors known answer + extra cases
    import contextlib
    import io
    cnt = np.array([[1, 19, 73], [1, 19, 90], [0, 33, 53], [5, 19, 91], [3, 17, 57], [3, 13, 77], [5, 6, 89], [1, 23, 85],
                    [2, 29, 67], [7, 6, 99], [0, 17, 96], [0, 10, 86], [4, 5, 85], [6, 25, 65], [0, 5, 86], [0, 16, 91],
                    [23, 14, 73], [4, 9, 96], [2, 19, 71], [9, 24, 78]])          # /root/reference/tests/test_dirichlet_multinomial.py:12
    with contextlib.redirect_stdout(io.StringIO()):
        fp = ref_dm.find_dirichlet_priors(cnt.astype(float), tol=1e-10, method="FP")
        loo = ref_dm.find_dirichlet_priors(cnt.astype(float), tol=1e-10, method="LOO")
        c4 = synth.allele_counts(3000, seed=9, depth=25, p_two=0.06).astype(float)
        fp4 = ref_dm.find_dirichlet_priors(c4, method="FPI", error_filt_threshold=0.01)
        fp4b = ref_dm.find_dirichlet_priors(c4[:40], method="FPI")
    out["find_dirichlet_priors"] = {"r_mglm": [20.8156311152126, 4.38181182238621, 0.889048781117318],
                                    "counts3": cnt.tolist(), "fp": list(map(float, fp)), "loo": list(map(float, loo)),
                                    "counts4_seed": 9, "fp4_filt0.01": list(map(float, fp4)), "fp4_first40": list(map(float, fp4b))}
    jdump("python_reference_golden.json", out)


# ---------------------------------------------------------------------------------------
# transcluster's p0 and E(K) from the series' definition at 40 digits (tests/hp_transcluster.py): neither the reference nor the
# oracle is used.  Keys: the CLI defaults' full cross of N x delta, and for every other (lamb, beta, thr) set two deltas per N,
# drawn with a fixed seed (every N boundary stays in).
HP_SETS = ((1e-3 * 29903, 73.0, 0.01),      # the CLI defaults
           (1e-3 * 29903, 73.0, 1e-6),      # the reference's own default threshold
           (5.3, 6.0, 0.01), (3.0, 52.0, 0.01),
           (20.0, 2.0, 0.05),               # short series
           (200.0, 150.0, 0.01),            # x = delta (lamb + beta) = 600 at 626 days; `upper` overflows near 3.5 years
           (0.5, 73.0, 0.01))               # k* = beta (N + 1) / lamb beyond the loop's 10 000 terms at small N
HP_N = (0, 1, 2, 7, 30, 127, 128, 129, 191, 192, 193, 1000, 1600, 3000, 4100, 6000, 8000, 9998, 9999, 10000, 10001, 15000,
        22766, 22767, 22768, 22769, 32766, 32767, 32768, 50000, 100000)
HP_GAPS = (0, 1, 2, 30, 365, 730, 1000, 2400, 9000)          # whole days: every route
HP_YEARS = (1e-9, 0.37, 3.3)                                  # deltas that are no whole number of days: the array routes only
HP_FIELDS = ("set", "N", "gap", "delta", "p0", "ln_eK", "k_stop", "cls", "k_lo", "k_hi", "ln_e_lo", "ln_e_hi", "ln_upper")


def _hp_one(args):
    import hp_transcluster as H
    s, N, gap, delta = args
    lamb, beta, thr = HP_SETS[s]
    r = H.evaluate(N, delta, lamb, beta, thr)
    return [s, N, gap, delta] + [r[f] for f in HP_FIELDS[4:]]


def hp_transcluster():
    import multiprocessing
    sys.path.insert(0, os.path.dirname(HERE))
    import hp_transcluster as H
    deltas = [(g, H.day_delta(g)) for g in HP_GAPS] + [(None, y) for y in HP_YEARS]
    rng = np.random.default_rng(20261016)
    work = []
    for s in range(len(HP_SETS)):
        for N in HP_N:
            pick = range(len(deltas)) if s == 0 else sorted(rng.choice(len(deltas), 2, replace=False).tolist())
            work += [(s, N) + deltas[i] for i in pick]
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        rows = pool.map(_hp_one, sorted(work, key=lambda w: -w[1]), chunksize=1)
    rows.sort(key=lambda r: (r[0], r[1], r[3]))
    out = {"about": "transcluster log P(direct) and E(K) from the series' definition at %d digits (tests/hp_transcluster.py); "
                    "delta = gap * 86400 / 31556952 in double for whole-day gaps" % H.DPS,
           "sets": [list(x) for x in HP_SETS], "fields": list(HP_FIELDS), "keys": rows}
    with open(os.path.join(HERE, "transcluster_hp_golden.json"), "w") as fh:
        fh.write(json.dumps({k: v for k, v in out.items() if k != "keys"})[:-1] + ', "keys": [\n')
        fh.write(",\n".join(json.dumps(r) for r in rows) + "\n]}\n")
    print("wrote transcluster_hp_golden.json", len(rows), "keys")


# ---------------------------------------------------------------------------------------
# The recombination filter's keep / drop boundary from its definition at 50 digits (tests/hp_filter.py).  One alignment per L; its
# sample s differs from sample 0 at the crafted sites of d_s.  What the d reach:
#   9 000:     the smallest d; L / (2 d) = 50 exactly (90: wh 51 against the clamp at 50, 91); dense p, where the binomial sum runs
#              on the lower side of the mean
#   120 000:   wh at 5 000 exactly (12); L / (2 d) = 1 500 exactly (40: the double rounding of 1.0 / p / 2.0 + 1); wh 51 against
#              50 (1 200, 1 201); spans clipped by 2 wh + 1
#   600 000:   wh clamped at 5 000 (45, 60) and the first d below the clamp (61); the bench workload's p = 980 / 5 M (118)
#   1 000 000: the bench workload's p again (196); the last table row and the first per-SNP one (65 536, 65 537); d far beyond
# A d whose sites held an ill cell would be replaced by d + 1 and said so here: none did.
FILTER_HP_CASES = ((9000, (2, 3, 90, 91, 600, 1500)),
                   (120000, (2, 7, 12, 37, 40, 300, 1200, 1201, 9000)),
                   (600000, (45, 60, 61, 118)),
                   (1000000, (196, 4200, 65536, 65537, 70000, 150000)))


def _hp_filter_one(args):
    import hp_filter as H
    L, d = args
    _, thr, wh = H.window(L, d)
    row = H.row(L, d)
    pos, covered = H.plan(L, d, row)
    kept, cells, ill, margin = H.filter_positions(pos, L)
    assert ill == 0, ("ill cell", L, d)
    hit = H.must_hit(L, d, row)
    assert all(c in cells for c in hit), ("the sites miss a boundary cell", L, d)
    # every k that has a boundary within reach of a window (n* <= 2 wh + 1; k = 2: <= wh + 1), up to 8 of them where d >= 600 and 2
    # where d >= 20: a sparse pair has no more than five or six such k (120 000 / 1 200: k = 2 .. 6), whatever the sites
    attainable = sum(n is not None and n <= (wh + 1 if k == 0 else 2 * wh + 1) for k, n in enumerate(row))
    assert len(covered) >= min(8 if d >= 600 else 2 if d >= 20 else 0, attainable), (L, d, covered)
    p = d / L
    ratio = 0.0
    with H.mp.workdps(H.DPS):
        for k, n in ((k + 2, n - e) for k, n in enumerate(row) if n is not None for e in (0, 1)):
            margin = min(margin, H.rel_margin(n, k, L, d))
            err = abs(H.mpf(1.0 - O.binomial_cdf(n, p, k)) - H.tail(n, k, p)) / H.mpf(thr)
            ratio = max(ratio, float(err))
    assert O.filter_recomb_positions(pos, L) == kept, ("oracle != definition", L, d)
    shape, at_wh, beyond = H.choose_probe(L, d)
    return {"L": L, "d": d, "wh": wh, "row": row, "min_margin": margin, "covered": len(covered), "attainable": attainable, "cells": len(cells),
            "expected": kept, "probe": [shape, at_wh, beyond]}, ratio


def hp_filter():
    import multiprocessing
    sys.path.insert(0, os.path.dirname(HERE))
    import hp_filter as H
    work = [(L, d) for L, ds in FILTER_HP_CASES for d in ds]
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        res = pool.map(_hp_filter_one, work, chunksize=1)
    cases = [r[0] for r in res]
    head = {"about": "the recombination filter's smallest surviving span n*(k), k = 2 .. 63, and the filtered distance of crafted pairs "
                     "(hp_filter.boundary_positions(L, d, row)) from the definition at %d digits (tests/hp_filter.py)" % H.DPS,
            "margin": H.MARGIN, "digits": H.DPS,
            "measured": {"min_relative_margin": min(c["min_margin"] for c in cases),
                         "oracle_max_error_over_threshold": float("%.2g" % max(r[1] for r in res)),
                         "ill_cells": 0,
                         "covered_per_case": {"%d/%d" % (c["L"], c["d"]): c["covered"] for c in cases}}}
    with open(os.path.join(HERE, "filter_hp_golden.json"), "w") as fh:
        fh.write(json.dumps(head)[:-1] + ', "cases": [\n')
        fh.write(",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    print("wrote filter_hp_golden.json", len(cases), "cases;", json.dumps(head["measured"]))


# ---------------------------------------------------------------------------------------
# The Dirichlet-multinomial prior fit from its definition at 50 digits, and the true values of digamma on a grid
# (tests/hp_dirichlet.py).  A case is a table of distinct rows with multiplicities (not a generator seed) plus the call's
# parameters; several cases share a table.  Tables whose name starts with "raw" hold rows as a caller would pass them (unsorted,
# unfiltered); the others hold kept rows, sorted ascending -- filtering them again changes nothing, so their cases may still pass a
# filter threshold.
def _dir_tables(H):
    t = {}

    def kept(c, filt=0.01):
        return H.distinct(np.sort(H.select_rows(np.asarray(c, np.float64), filt), axis=1))
    t["d8"] = kept(synth.allele_counts(3000, seed=21, depth=8, p_two=0.06))
    t["d25"] = kept(synth.allele_counts(3000, seed=9, depth=25, p_two=0.06))
    t["d200"] = kept(synth.allele_counts(1000, seed=23, depth=200, p_two=0.06))
    for name, seed, scale in (("c60k", 24, 500), ("c3e8", 25, 2500000)):      # per-allele counts near 60 000 and near 3e8
        rng = np.random.default_rng(seed)
        c = synth.allele_counts(300, seed=seed, depth=120, p_two=0.1).astype(np.int64)
        t[name] = kept(c * scale + (c > 0) * rng.integers(0, scale, c.shape))
    for K in (2, 3, 5, 8):                                                     # K alleles at depth 25, probabilities ~ 0.7 ** k
        rng = np.random.default_rng(30 + K)
        p = 0.7 ** np.arange(K)
        c = np.array([rng.multinomial(n, p / p.sum()) for n in rng.poisson(25, {2: 2000, 3: 600, 5: 300, 8: 300}[K])])
        t["k%d" % K] = kept(c, None)
    rng = np.random.default_rng(40)                                            # K = 4, two alleles only
    dep = rng.poisson(25, 2000)
    b = rng.binomial(dep, rng.beta(0.6, 1.4, 2000))                            # overdispersed: the fit converges within max_iter
    t["two"] = kept(np.stack([b, dep - b, 0 * b, 0 * b], 1), None)
    d25 = t["d25"]
    t["cut5"] = [r[:-1] + [1] for r in d25[:5]]
    t["cut6"] = [r[:-1] + [1] for r in d25[:6]]
    # the filter at equality: 1 / 20 == 0.05 is not < 0.05 (kept); 1 / 40 is (the cell becomes 0: one allele left, dropped);
    # a row without counts divides 0 / 0 and stays as it is (dropped)
    base = [r for r in d25[:120]]
    t["raw_base"] = base              # the variants add one row each (the cases' extra_rows)
    return t


def _dir_cases():
    c = []
    for tab in ("d8", "d25", "d200"):
        for method in ("FPI", "LOO"):
            for tol in (1e-5, 1e-11):
                c.append(dict(name="%s_%s_%g" % (tab, method, tol), table=tab, method=method, tol=tol, max_iter=1000,
                              error_filt_threshold=0.01 if method == "FPI" else None))
    for tab in ("c60k", "c3e8"):
        c.append(dict(name=tab, table=tab, method="FPI", tol=1e-5, max_iter=1000, error_filt_threshold=0.01))
    for K in (2, 3, 5, 8):
        c.append(dict(name="k%d" % K, table="k%d" % K, method="FPI", tol=1e-5, max_iter=1000, error_filt_threshold=None))
    c.append(dict(name="two_converged", table="two", method="FPI", tol=1e-5, max_iter=1000, error_filt_threshold=None))
    c.append(dict(name="two_max_iter", table="two", method="FPI", tol=1e-5, max_iter=40, error_filt_threshold=None))
    for mi in (0, 1, 31, 32, 33, 64, 65):
        c.append(dict(name="d25_max_iter_%d" % mi, table="d25", method="FPI", tol=1e-5, max_iter=mi, error_filt_threshold=0.01))
    for tab in ("cut5", "cut6"):
        c.append(dict(name=tab, table=tab, method="FPI", tol=1e-5, max_iter=1000, error_filt_threshold=None))
    for name, extra in (("base", []), ("keep19", [[19, 1, 0, 0, 400]]), ("drop39", [[39, 1, 0, 0, 400]]), ("zero", [[0, 0, 0, 0, 400]])):
        c.append(dict(name=name + "_filter_0.05", table="raw_base", extra_rows=extra, method="FPI", tol=1e-5, max_iter=1000,
                      error_filt_threshold=0.05))
    return c


def _hp_dirichlet_one(args):
    import hp_dirichlet as H
    case, table = args
    rows = H.expand(table + case.get("extra_rows", []))
    K = rows.shape[1]
    keptrows = H.select_rows(rows, case["error_filt_threshold"])
    out = dict(case, K=K, kept_rows=int(len(keptrows)))
    if len(keptrows) <= 5:
        alphas, iters, margin = [0] * (K - 1) + [1], 0, None
        out.update(alphas=[[float(a), 0.0] for a in alphas], iters=0, margin=None)
    else:
        d = np.array(H.distinct(np.sort(keptrows, axis=1)), np.float64)
        alphas, iters, margin = H.hp_fit(d[:, :-1], case["max_iter"], case["tol"], case["method"], mult=d[:, -1])
        assert margin is None or margin >= H.ILL, ("ill case", case["name"], margin)
        out.update(alphas=[H.split(a) for a in alphas], iters=iters, margin=margin)
    got, oit = O.find_dirichlet_priors(rows, max_iter=case["max_iter"], tol=case["tol"], method=case["method"],
                                       error_filt_threshold=case["error_filt_threshold"], return_iters=True)
    assert oit == out["iters"], ("the oracle stops elsewhere", case["name"], oit, out["iters"])
    hi, lo = np.array(out["alphas"]).T
    out["oracle_rel_err"] = float(H.rel_errors(got, hi, lo).max())
    return out


def hp_dirichlet():
    import multiprocessing
    from scipy.special import psi
    sys.path.insert(0, os.path.dirname(HERE))
    import hp_dirichlet as H
    tables = _dir_tables(H)
    cases = _dir_cases()
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        res = pool.map(_hp_dirichlet_one, [(c, tables[c["table"]]) for c in cases], chunksize=1)
    xs = H.digamma_grid()
    hi, lo = H.digamma_true(xs)
    scipy_worst = float(np.abs(H.ulp_errors(psi(xs), hi, H.digamma_lo(hi, lo))).max())
    head = {"about": "find_dirichlet_priors (alphas, iterations) and digamma from their definitions at %d digits (tests/hp_dirichlet.py); "
                     "a value is [nearest double, double of the remainder]; digamma_lo_ulp: the remainder in units of ulp(digamma_hi)" % H.DPS,
            "digits": H.DPS, "ill": H.ILL,
            "digamma": {"points": len(xs), "x_first_last": [float(xs[0]), float(xs[-1])], "x_sum": float(np.sum(xs)),
                        "scipy_worst_ulp": float("%.3g" % scipy_worst)}}
    with open(os.path.join(HERE, "dirichlet_hp_golden.json"), "w") as fh:
        fh.write(json.dumps(head)[:-1] + ',\n"digamma_hi": ' + json.dumps(hi) + ',\n"digamma_lo_ulp": ' + json.dumps(lo) + ',\n"tables": {\n')
        fh.write(",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in tables.items()) + '\n},\n"cases": [\n')
        fh.write(",\n".join(json.dumps(c) for c in res) + "\n]}\n")
    print("wrote dirichlet_hp_golden.json", len(res), "cases; scipy's psi worst %.3g ulp" % scipy_worst)
    for c in res:
        print("  %-22s kept %5d  iters %4d  margin %-10s oracle_rel_err %.3g" % (c["name"], c["kept_rows"], c["iters"],
                                                                                 "%.3g" % c["margin"] if c["margin"] is not None else "-", c["oracle_rel_err"]))


if __name__ == "__main__":
    if sys.argv[1:] == ["hp-dirichlet"]:         # only the high-precision fit / digamma fixture (no reference needed)
        hp_dirichlet()
        sys.exit(0)
    if sys.argv[1:] == ["hp-filter"]:            # only the high-precision filter fixture (no reference needed)
        hp_filter()
        sys.exit(0)
    if sys.argv[1:] == ["hp-transcluster"]:     # only the high-precision transcluster fixture (no reference, no oracle needed)
        hp_transcluster()
        sys.exit(0)
    if sys.argv[1:] == ["outbreak"]:             # only the fixture added in round 3
        transcluster_outbreak()
        sys.exit(0)
    if sys.argv[1:] == ["large-n"]:              # only the fixture added in round 2
        transcluster_large_n()
        sys.exit(0)
    if sys.argv[1:] == ["pairsnp-ref"]:          # only the fixture of tests/test_pairsnp_ref.py / tests/test_gpu_pairsnp_ref.py
        pairsnp_ref()
        sys.exit(0)
    if sys.argv[1:] == ["python-reference"]:     # only the Python drivers' golden
        python_reference()
        sys.exit(0)
    if sys.argv[1:] == ["pairsnp-unpinned"]:
        pairsnp_unpinned()
        sys.exit(0)
    if sys.argv[1:] == ["oracle-vs-ref"]:        # only the fixture of tests/test_oracle_vs_ref.py
        oracle_vs_ref()
        sys.exit(0)
    transcluster()
    transcluster_large_n()
    posteriors()
    kseq()
    pairsnp_unpinned()
    pairsnp_ref()
    python_reference()
