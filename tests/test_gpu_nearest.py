"""Per-sample k nearest neighbours (tracs_nearest, tracs_knn_*: csrc/nearest.hip) against the oracle's all pairs, ranked by
(SNP distance, sample index) and cut to k per sample.  Every comparison is bit-exact on rows, cols, d and nn."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def expected(O, seqs, k, n0=None, dist=2147483647):
    """rows, cols, d, nn of each sample's k nearest, from the oracle's pairs."""
    r, c, d, nn = O.pairsnp_arrays(seqs, n0=n0, dist=dist, n_threads=8)
    if n0 is None:                                   # one file: a pair is a candidate of both of its samples
        r, c, d, nn = np.concatenate([r, c]), np.concatenate([c, r]), np.concatenate([d, d]), np.concatenate([nn, nn])
    o = np.lexsort((c, d, r))
    r, c, d, nn = r[o], c[o], d[o], nn[o]
    keep = np.arange(len(r)) - np.searchsorted(r, r) < k
    return r[keep], c[keep], d[keep], nn[keep]


def check(got, exp, what):
    for name, g, e in zip(("rows", "cols", "d", "nn"), got, exp):
        g = np.asarray(g).astype(np.uint64)
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        assert np.array_equal(g, e), (what, name, np.flatnonzero(g != e)[:5])


def seqs_for(n, L, seed, **kw):
    from tracs_amd import synth
    args = dict(mu_lineage=3e-3, mu_sample=1e-3, p_n=0.02, p_partial=0.005)
    args.update(kw)
    return synth.alignment(n, L, seed=seed, **args)


def nearest(tmp_path, seqs, k, dist=2147483647, filter=False, db=None):
    from tracs_amd import api, synth
    fa = str(tmp_path / "q.fa")
    synth.write_fasta(fa, seqs)
    paths = [fa]
    if db is not None:
        paths.append(str(tmp_path / "db.fa"))
        synth.write_fasta(paths[1], db, names=["db%d" % i for i in range(db.shape[0])])
    r, c, d, names, f, nn = api.nearest_arrays(paths, k, dist=dist, filter=filter)
    return (r, c, d, nn), f, names


SHAPES = [(2, 1), (5, 37), (65, 1000), (130, 4097), (300, 20000)]


@pytest.mark.parametrize("n,L", SHAPES, ids=lambda v: str(v))
def test_nearest_shapes_and_k(hiplib, oracle, tmp_path, n, L):
    seqs = seqs_for(n, L, seed=n * 31 + L)
    for k in sorted({1, 3, 16, max(n - 1, 1), n + 5}):
        got, f, names = nearest(tmp_path, seqs, k)
        check(got, expected(oracle, seqs, k), (n, L, k))
        assert len(names) == n and np.array_equal(np.asarray(f), np.zeros(len(got[0]), np.uint64))
        assert len(got[0]) == n * min(k, n - 1)


def test_nearest_heavy_ties(hiplib, oracle, tmp_path):
    seqs = seqs_for(200, 3000, seed=5, n_lineages=4)
    for g in range(0, 200, 20):                       # groups of identical sequences: every key of a group ties on d
        seqs[g + 1:g + 12] = seqs[g]
    for k in (1, 5, 11, 16, 64, 199):
        got, _, _ = nearest(tmp_path, seqs, k)
        check(got, expected(oracle, seqs, k), ("ties", k))


def test_nearest_two_files(hiplib, oracle, tmp_path):
    allseqs = seqs_for(170, 5000, seed=11, n_lineages=6)
    q, db = allseqs[:40], allseqs[40:]
    for k in (1, 7, 130, 200):
        got, _, names = nearest(tmp_path, q, k, db=db)
        exp = expected(oracle, allseqs, k, n0=40)
        check(got, exp, ("two files", k))
        assert len(names) == 170 and set(np.asarray(got[0]).tolist()) <= set(range(40))
        assert (np.asarray(got[1]) >= 40).all()


def test_nearest_threshold(hiplib, oracle, tmp_path):
    seqs = seqs_for(250, 8000, seed=13, n_lineages=8, mu_lineage=1e-2)
    _, _, d_all, _ = oracle.pairsnp_arrays(seqs, n_threads=8)
    for q in (1, 10, 40):
        thr = int(np.percentile(d_all, q))
        for k in (4, 32):
            got, _, _ = nearest(tmp_path, seqs, k, dist=thr)
            exp = expected(oracle, seqs, k, dist=thr)
            check(got, exp, ("-D", thr, k))
            counts = np.bincount(exp[0].astype(np.int64), minlength=250)
            if q == 1:
                assert (counts < k).any()              # samples with fewer than k eligible candidates


def test_nearest_filter(hiplib, oracle, tmp_path):
    from tracs_amd import api, synth
    seqs = seqs_for(90, 20000, seed=17, n_lineages=3)
    fa = str(tmp_path / "f.fa")
    synth.write_fasta(fa, seqs)
    r, c, d, _, f, nn = api.nearest_arrays([fa], 6, filter=True)
    check((r, c, d, nn), expected(oracle, seqs, 6), "filter")
    ar, ac, ad, _, af, _ = api.pairsnp_arrays([fa], filter=True)
    filt = {(int(a), int(b)): int(x) for a, b, x in zip(ar, ac, af)}
    want = [filt[(min(int(a), int(b)), max(int(a), int(b)))] for a, b in zip(r, c)]
    assert np.array_equal(np.asarray(f, np.uint64), np.asarray(want, np.uint64))


def test_knn_update_panel_splits(hiplib, oracle):
    import torch

    from tracs_amd import device as dev
    n, L, k = 150, 6000, 9
    seqs = seqs_for(n, L, seed=19, n_lineages=5)
    seqs[10:20] = seqs[9]
    aln = dev.Alignment(n, L)
    aln.pack(seqs)
    d = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    nn = torch.zeros_like(d)
    dev.pairsnp_dense(aln, d, nn)
    exp = expected(oracle, seqs, k)
    for split in (1, 7, 64, n):
        state = dev.knn_init(n, k)
        for r0 in range(0, n, split):
            dev.knn_update(state, d, nn, n, k, row_begin=r0, row_end=min(n, r0 + split))
        got = [t.cpu().numpy().astype(np.uint32) for t in dev.knn_emit(state, k, 0, n)]
        check(got, exp, ("split", split))
    # emit of a sub-range of the lists, and panels held as separate buffers (absolute row indexing through base_row)
    state = dev.knn_init(n, k)
    for r0 in range(0, n, 64):
        r1 = min(n, r0 + 64)
        pd, pn = d[r0:r1].clone(), nn[r0:r1].clone()
        dev.knn_update(state, pd, pn, n, k, row_begin=r0, row_end=r1, base_row=r0)
    got = [t.cpu().numpy().astype(np.uint32) for t in dev.knn_emit(state, k, 30, 80)]
    sel = (exp[0] >= 30) & (exp[0] < 80)
    check(got, [e[sel] for e in exp], "sub-range")
    aln.close()


def seam_distances(n, xp):
    """The scan-seam test's d[i][j], symmetric and in [0, max(5, n // 2)), from the indices alone; xp: numpy or torch-on-the-device
    (arange, minimum, maximum).  About 4 partners of a sample have d <= 1, so lists of every length up to k = 3 occur."""
    i, j = xp.arange(n).reshape(n, 1), xp.arange(n).reshape(1, n)
    lo, hi = xp.minimum(i, j), xp.maximum(i, j)
    return (lo * 7919 + hi * 104729 + lo * hi) % 1000003 % max(5, n // 2)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2048, 2049])
def test_knn_emit_at_scan_seams(hiplib, n):
    """tracs_knn_emit scans the lists' lengths in one workgroup that steps by 1 024 and writes the total at index n: n on, one below
    and one above a multiple of the step, and more than one step.  The lists come from a formula, the expected ones from NumPy."""
    import torch

    from tracs_amd import device as dev
    k, thr, ncomp = 3, 1, 777
    D = seam_distances(n, np)
    mask = (D <= thr) & ~np.eye(n, dtype=bool)
    lengths = np.minimum(mask.sum(axis=1), k)
    if n >= 1023:                                       # the offsets are not a constant stride
        assert set(np.unique(lengths).tolist()) == {0, 1, 2, 3}
    r, c = np.nonzero(mask)
    o = np.lexsort((c, D[r, c], r))
    r, c = r[o], c[o]
    keep = np.arange(len(r)) - np.searchsorted(r, r) < k
    exp = [r[keep], c[keep], D[r, c][keep], np.full(int(keep.sum()), ncomp)]
    assert len(exp[0]) == int(lengths.sum())
    class on_device:                                    # int64 index arithmetic on the GPU
        arange = staticmethod(lambda m: torch.arange(m, dtype=torch.int64, device="cuda"))
        minimum, maximum = torch.minimum, torch.maximum
    d = seam_distances(n, on_device).to(torch.int32).contiguous()
    nn = torch.full((n, n), ncomp, dtype=torch.int32, device="cuda")
    state = dev.knn_init(n, k)
    dev.knn_update(state, d, nn, n, k, dist_threshold=thr)
    got = [t.cpu().numpy().astype(np.uint32) for t in dev.knn_emit(state, k, 0, n)]
    check(got, [np.asarray(e).astype(np.uint64) for e in exp], ("scan seam", n))


@pytest.mark.parametrize("k", [100, 300])
def test_knn_update_panel_splits_large_k(hiplib, oracle, k):
    """K > 64: both parts merge into the lists in the state (wave_merge, four / sixteen entries per lane), the column part reads nn
    of the keys it kept after its walk; row panels of their own, at offsets other than 0."""
    import torch

    from tracs_amd import device as dev
    n, L = 400, 3000
    seqs = seqs_for(n, L, seed=k, n_lineages=6)
    seqs[50:70] = seqs[49]
    aln = dev.Alignment(n, L)
    aln.pack(seqs)
    d = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    nn = torch.zeros_like(d)
    dev.pairsnp_dense(aln, d, nn)
    exp = expected(oracle, seqs, k)
    for split in (7, 150, n):
        state = dev.knn_init(n, k)
        for r0 in range(0, n, split):
            r1 = min(n, r0 + split)
            dev.knn_update(state, d[r0:r1].clone(), nn[r0:r1].clone(), n, k, row_begin=r0, row_end=r1, base_row=r0)
        got = [t.cpu().numpy().astype(np.uint32) for t in dev.knn_emit(state, k, 0, n)]
        check(got, exp, ("split", split, "k", k))
    aln.close()


ROUTE_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from tracs_amd import api, device as dev, synth
out = {}
for n, L, p_partial in ((120, 30000, 0.0), (120, 30000, 0.003)):
    seqs = synth.alignment(n, L, seed=n + L + int(p_partial * 1e4), mu_lineage=2e-3, mu_sample=3e-4, n_lineages=4, p_n=0.02,
                           p_partial=p_partial, p_other=0.001)
    fa = "%(tmp)s/route_%%d.fa" %% int(p_partial * 1e4)
    synth.write_fasta(fa, seqs)
    r, c, d, _, _, nn = api.nearest_arrays([fa], 12)
    out["p%%d" %% int(p_partial * 1e4)] = np.stack([np.asarray(x, np.uint64) for x in (r, c, d, nn)])
    aln = dev.Alignment(n, L); aln.pack(seqs)
    dd = torch.zeros((n, n), dtype=torch.int32, device="cuda"); dev.pairsnp_dense(aln, dd, None)
    out["kernel%%d" %% int(p_partial * 1e4)] = np.array([aln.kernel == "valu", aln.site_classes is not None])
    aln.close()
np.savez(sys.argv[1], **out)
'''

ROUTES = [{"TRACS_SITE_CLASSES": "1"}, {"TRACS_SITE_CLASSES": "0"}, {"TRACS_MFMA": "0"}]


def test_nearest_same_on_every_route(hiplib, oracle, tmp_path):
    from tracs_amd import synth
    res = []
    for env in ROUTES:
        npz = str(tmp_path / ("r%d.npz" % len(res)))
        out = subprocess.run([sys.executable, "-c", ROUTE_CHILD % {"root": ROOT, "tmp": str(tmp_path)}, npz], capture_output=True,
                             text=True, env=dict(os.environ, **env), timeout=300, cwd=ROOT)
        assert out.returncode == 0, (env, out.stdout[-1500:] + out.stderr[-3000:])
        res.append(dict(np.load(npz)))
    assert res[0]["kernel0"][1] and not res[1]["kernel0"][1] and res[2]["kernel0"][0]      # the routes were the ones asked for
    for p in (0, 30):
        seqs = synth.alignment(120, 30000, seed=120 + 30000 + p, mu_lineage=2e-3, mu_sample=3e-4, n_lineages=4, p_n=0.02,
                               p_partial=p / 1e4, p_other=0.001)
        exp = np.stack(expected(oracle, seqs, 12))
        for env, r in zip(ROUTES, res):
            assert np.array_equal(r["p%d" % p], exp), (env, p)


def test_nearest_large_against_oracle(hiplib, oracle, tmp_path):
    """~2 000 x 200 kbp with lineages, through several row panels of the device primitives."""
    import torch

    from tracs_amd import device as dev
    n, L, k = 2000, 200000, 10
    seqs = seqs_for(n, L, seed=23, n_lineages=40, mu_lineage=5e-4, mu_sample=5e-5, p_n=0.01, p_partial=0.0005)
    aln = dev.Alignment(n, L)
    aln.pack(seqs)
    state = dev.knn_init(n, k)
    panel = 700
    d = torch.empty((panel, n), dtype=torch.int32, device="cuda")
    nn = torch.empty_like(d)
    for r0 in range(0, n, panel):
        r1 = min(n, r0 + panel)
        dev.pairsnp_dense(aln, d, nn, row_begin=r0, row_end=r1, dist_threshold=2147483647, base_row=r0)
        dev.knn_update(state, d, nn, n, k, row_begin=r0, row_end=r1, base_row=r0)
    got = [t.cpu().numpy().astype(np.uint32) for t in dev.knn_emit(state, k, 0, n)]
    aln.close()
    check(got, expected(oracle, seqs, k), "2000 x 200 kbp")


def test_nearest_cli_meta_and_cluster(hiplib, oracle, tmp_path):
    from tracs_amd import api, synth
    n, L, k = 80, 20000, 5
    seqs = seqs_for(n, L, seed=29, n_lineages=4, mu_lineage=2e-4, mu_sample=1e-4)
    names = ["iso%d" % i for i in range(n)]
    fa = str(tmp_path / "refX_combined.fasta")
    synth.write_fasta(fa, seqs, names=names)
    iso, days = synth.dates(n, seed=29)
    meta = str(tmp_path / "meta.csv")
    with open(meta, "w") as fh:
        fh.write("sample,date\n")
        for nm, s in zip(names, iso):
            fh.write("%s,%s\n" % (nm, s))
    out = str(tmp_path / "near.csv")
    lamb, beta = 5.3, 6.0
    r, c, d, nn = expected(oracle, seqs, k)
    delta = np.abs(days[r.astype(np.int64)] - days[c.astype(np.int64)]).astype(np.float64) * 86400.0 / 31556952.0
    p0, ek = api.trans_dist_arrays(d.astype(np.int32), delta, lamb, beta, 0.01)
    kmax = max(1, int(np.percentile(ek, 50)))                # -K drops rows after the selection
    keep = ek <= kmax
    cmd = [sys.executable, "-m", "tracs_amd", "distance", "--msa", fa, "--meta", meta, "-o", out, "--nearest", str(k),
           "--clock_rate", str(lamb), "--trans_rate", str(beta), "-K", str(kmax), "--loglevel", "ERROR"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    assert keep.any()
    lines = open(out).read().strip().split("\n")
    assert lines[0].startswith("sampleA,sampleB,date difference")
    rows = [ln.split(",") for ln in lines[1:]]
    assert len(rows) == int(keep.sum())
    idx = {nm: i for i, nm in enumerate(names)}
    for f, i, j, dd, pp, e, m, dl in zip(rows, r[keep], c[keep], d[keep], np.exp(p0[keep]), ek[keep], nn[keep], delta[keep]):
        assert (idx[f[0]], idx[f[1]], int(f[3]), int(f[7])) == (int(i), int(j), int(dd), int(m))
        assert float(f[2]) == dl and float(f[4]) == pp and float(f[5]) == e
        assert f[6] == "NA" and f[8] == "refX"
    cl = str(tmp_path / "clusters.csv")
    p = subprocess.run([sys.executable, "-m", "tracs_amd", "cluster", "-d", out, "-o", cl, "-c", "10", "-D", "snp", "--loglevel", "ERROR"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    assert os.path.getsize(cl) > 0
