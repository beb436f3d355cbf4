"""SNP distance histograms on the GPU (tracs_hist_*, tracs_distance_histogram: csrc/histogram.hip) against
np.bincount over the oracle's pairs, class by class.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("within", "between", "ungrouped")


def classes_of(labels, r, c):
    """0 within, 1 between, 2 ungrouped for the pairs (r, c); labels None: all ungrouped."""
    if labels is None:
        return np.full(len(r), 2, np.int64)
    gi, gj = labels[r.astype(np.int64)], labels[c.astype(np.int64)]
    return np.where((gi < 0) | (gj < 0), 2, np.where(gi == gj, 0, 1)).astype(np.int64)


def bincount_hist(values, cls):
    """-> value, within, between, ungrouped of the non-empty bins, ascending."""
    values = np.asarray(values).astype(np.int64)
    if not len(values):
        return [np.zeros(0, np.uint64)] * 4
    m = int(values.max()) + 1
    counts = [np.bincount(values[cls == k], minlength=m) for k in range(3)]
    used = np.flatnonzero(counts[0] + counts[1] + counts[2])
    return [used.astype(np.uint64)] + [c[used].astype(np.uint64) for c in counts]


def expected(O, seqs, labels=None, n0=None, dist=2147483647):
    r, c, d, _ = O.pairsnp_arrays(seqs, n0=n0, dist=dist, n_threads=8)
    return bincount_hist(d, classes_of(labels, r, c)), len(r)


def check(got, exp, what):
    """got: dict value/within/between/ungrouped, or a list in that order."""
    if isinstance(got, dict):
        got = [got["value"], got["within"], got["between"], got["ungrouped"]]
    for name, g, e in zip(("value",) + CLASSES, got, exp):
        g = np.asarray(g).astype(np.uint64)
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        assert np.array_equal(g, e), (what, name, np.flatnonzero(g != e)[:5])


def seqs_for(n, L, seed, **kw):
    from tracs_amd import synth
    args = dict(mu_lineage=3e-3, mu_sample=1e-3, p_n=0.02, p_partial=0.005)
    args.update(kw)
    return synth.alignment(n, L, seed=seed, **args)


def random_labels(n, seed):
    """Ungrouped samples, singleton groups and one group that holds most samples."""
    rng = np.random.default_rng(seed)
    lab = np.zeros(n, np.int32)                                  # group 0: most samples
    k = max(1, n // 5)
    lab[rng.choice(n, k, replace=False)] = rng.integers(1, 4, k).astype(np.int32)
    singles = rng.choice(n, max(1, n // 10), replace=False)
    lab[singles] = 100 + np.arange(len(singles), dtype=np.int32)  # singleton groups
    lab[rng.choice(n, max(1, n // 8), replace=False)] = -1         # ungrouped
    return lab


def groups_of(names, lab):
    return {nm: ("g%d" % g) for nm, g in zip(names, lab) if g >= 0}


def histogram(tmp_path, seqs, labels=None, dist=2147483647, filter=False, db=None):
    from tracs_amd import api, synth
    fa = str(tmp_path / "q.fa")
    names = ["s%d" % i for i in range(seqs.shape[0])]
    synth.write_fasta(fa, seqs, names=names)
    paths = [fa]
    if db is not None:
        paths.append(str(tmp_path / "db.fa"))
        names = names + ["db%d" % i for i in range(db.shape[0])]
        synth.write_fasta(paths[1], db, names=names[seqs.shape[0]:])
    got_names, h = api.distance_histogram(paths, dist=dist, filter=filter, groups=None if labels is None else groups_of(names, labels))
    assert got_names == names
    return h


SHAPES = [(2, 1), (5, 37), (65, 1000), (130, 4097), (300, 20000)]


@pytest.mark.parametrize("n,L", SHAPES, ids=lambda v: str(v))
def test_histogram_shapes_with_and_without_groups(hiplib, oracle, tmp_path, n, L):
    seqs = seqs_for(n, L, seed=n * 31 + L)
    exp, pairs = expected(oracle, seqs)
    assert pairs == n * (n - 1) // 2
    h = histogram(tmp_path, seqs)
    check(h["snp"], exp, (n, L, "no groups"))
    assert "filter" not in h and not h["snp"]["within"].any() and not h["snp"]["between"].any()
    lab = random_labels(n, seed=n)
    exp, pairs = expected(oracle, seqs, lab)
    h = histogram(tmp_path, seqs, lab)["snp"]
    check(h, exp, (n, L, "groups"))
    assert int(h["within"].sum() + h["between"].sum() + h["ungrouped"].sum()) == pairs
    if n >= 65:
        assert h["within"].any() and h["between"].any() and h["ungrouped"].any()


def test_histogram_two_files(hiplib, oracle, tmp_path):
    allseqs = seqs_for(170, 5000, seed=11, n_lineages=6)
    lab = random_labels(170, seed=3)
    h = histogram(tmp_path, allseqs[:40], lab, db=allseqs[40:])["snp"]
    exp, pairs = expected(oracle, allseqs, lab, n0=40)
    check(h, exp, "two files")
    assert pairs == 40 * 130 == int(h["within"].sum() + h["between"].sum() + h["ungrouped"].sum())     # only cross pairs
    check(histogram(tmp_path, allseqs[:40], None, db=allseqs[40:])["snp"], expected(oracle, allseqs, None, n0=40)[0], "two files, no groups")


def test_histogram_threshold(hiplib, oracle, tmp_path):
    seqs = seqs_for(250, 8000, seed=13, n_lineages=8, mu_lineage=1e-2)
    lab = random_labels(250, seed=5)
    _, _, d_all, _ = oracle.pairsnp_arrays(seqs, n_threads=8)
    for q in (1, 10, 40):
        thr = int(np.percentile(d_all, q))
        exp, pairs = expected(oracle, seqs, lab, dist=thr)
        h = histogram(tmp_path, seqs, lab, dist=thr)["snp"]
        check(h, exp, ("-D", thr))
        assert pairs == int((d_all <= thr).sum()) and int(h["value"].max()) <= thr


ROUTE_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from tracs_amd import api, device as dev, synth
out = {}
n, L = 120, 30000
thrs = [int(x) for x in sys.argv[2:]]
seqs = synth.alignment(n, L, seed=n + L, mu_lineage=2e-3, mu_sample=3e-4, n_lineages=4, p_n=0.02, p_other=0.001)
lab = np.load("%(tmp)s/labels.npy")
fa = "%(tmp)s/route.fa"
names = ["s%%d" %% i for i in range(n)]
synth.write_fasta(fa, seqs, names=names)
groups = {nm: int(g) for nm, g in zip(names, lab) if g >= 0}
for thr in thrs:
    _, h = api.distance_histogram([fa], dist=thr, groups=groups)
    out["t%%d" %% thr] = np.stack([np.asarray(h["snp"][k], np.uint64) for k in ("value", "within", "between", "ungrouped")])
aln = dev.Alignment(n, L); aln.pack(seqs)
dd = torch.zeros((n, n), dtype=torch.int32, device="cuda"); dev.pairsnp_dense(aln, dd, None)
out["kernel"] = np.array([aln.kernel == "valu", aln.site_classes is not None])
aln.close()
np.savez(sys.argv[1], **out)
'''

ROUTES = [{"TRACS_SITE_CLASSES": "1"}, {"TRACS_SITE_CLASSES": "0"}, {"TRACS_MFMA": "0"}]


def test_histogram_threshold_same_on_every_pair_route(hiplib, oracle, tmp_path):
    """On the thresholded pair routes the cells past -D hold values that are not distances: none of them may be counted."""
    from tracs_amd import synth
    n, L = 120, 30000
    seqs = synth.alignment(n, L, seed=n + L, mu_lineage=2e-3, mu_sample=3e-4, n_lineages=4, p_n=0.02, p_other=0.001)
    lab = random_labels(n, seed=7)
    np.save(str(tmp_path / "labels.npy"), lab)
    _, _, d_all, _ = oracle.pairsnp_arrays(seqs, n_threads=8)
    thrs = sorted({int(np.percentile(d_all, q)) for q in (1, 10, 40)})
    res = []
    for env in ROUTES:
        npz = str(tmp_path / ("r%d.npz" % len(res)))
        out = subprocess.run([sys.executable, "-c", ROUTE_CHILD % {"root": ROOT, "tmp": str(tmp_path)}, npz] + [str(t) for t in thrs],
                             capture_output=True, text=True, env=dict(os.environ, **env), timeout=300, cwd=ROOT)
        assert out.returncode == 0, (env, out.stdout[-1500:] + out.stderr[-3000:])
        res.append(dict(np.load(npz)))
    assert res[0]["kernel"][1] and not res[1]["kernel"][1] and res[2]["kernel"][0]      # the routes were the ones asked for
    for thr in thrs:
        exp, _ = expected(oracle, seqs, lab, dist=thr)
        for env, r in zip(ROUTES, res):
            check(list(r["t%d" % thr]), exp, (env, thr))


def dense_panel(seqs):
    import torch

    from tracs_amd import device as dev
    n, L = seqs.shape
    aln = dev.Alignment(n, L)
    aln.pack(seqs)
    d = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    nn = torch.zeros_like(d)
    dev.pairsnp_dense(aln, d, nn)
    return aln, d, nn


def emitted(state, n_bins):
    from tracs_amd import device as dev
    v, w, b, u = dev.hist_emit(state, n_bins)
    return [v.cpu().numpy().astype(np.uint32).astype(np.uint64)] + [t.cpu().numpy().astype(np.uint64) for t in (w, b, u)]


def test_hist_update_panel_splits(hiplib, oracle):
    import torch

    from tracs_amd import device as dev
    n, L = 150, 6000
    seqs = seqs_for(n, L, seed=19, n_lineages=5)
    seqs[10:20] = seqs[9]
    lab = random_labels(n, seed=9)
    aln, d, nn = dense_panel(seqs)
    g = torch.from_numpy(lab).cuda()
    n_bins = L + 1
    for labels, group in ((lab, g), (None, None)):
        exp, _ = expected(oracle, seqs, labels)
        states = []
        for split in (n, 7, 64, 1):                       # one panel, uneven row panels, panels of one row
            state = dev.hist_init(n_bins)
            for r0 in range(0, n, split):
                dev.hist_update(state, n_bins, d, n, row_begin=r0, row_end=min(n, r0 + split), group=group)
            check(emitted(state, n_bins), exp, ("split", split, labels is not None))
            states.append(state)
        # the same state: header word 0 (values out of range) and every bin, bit for bit
        words = [s.view(torch.int64) for s in states]
        for wds in words[1:]:
            assert int(wds[0].item()) == 0 and torch.equal(wds[8:8 + 3 * n_bins], words[0][8:8 + 3 * n_bins])
        # panels held as separate buffers (absolute row indexing through base_row), a column offset, and a threshold
        state = dev.hist_init(n_bins)
        for r0 in range(0, n, 64):
            r1 = min(n, r0 + 64)
            dev.hist_update(state, n_bins, d[r0:r1].clone(), n, row_begin=r0, row_end=r1, group=group, base_row=r0)
        check(emitted(state, n_bins), exp, "separate buffers")
        state = dev.hist_init(n_bins)
        dev.hist_update(state, n_bins, d, n, row_begin=0, row_end=40, col_begin=40, group=group)
        check(emitted(state, n_bins), expected(oracle, seqs, labels, n0=40)[0], "col_begin")
        # the listed pairs of the same panel, in three batches, give the same histogram
        rows, cols, dd, _ = dev.coo_from_dense(d, nn, n)
        state = dev.hist_init(n_bins)
        m = rows.numel()
        for a, b in ((0, 1), (1, m // 3), (m // 3, m)):
            dev.hist_update_coo(state, n_bins, rows[a:b].contiguous(), cols[a:b].contiguous(), dd[a:b].contiguous(), group=group)
        check(emitted(state, n_bins), exp, "coo")
    aln.close()


@pytest.mark.parametrize("n_bins", [1023 * 1024, 1024 * 1024, 1024 * 1024 + 1, 2048 * 1024 + 1])
def test_hist_emit_at_scan_seams(hiplib, n_bins):
    """tracs_hist_emit scans the per-chunk counts of non-empty bins (chunks of 1 024 bins) in one workgroup that steps by 1 024 and
    writes the total at index `chunks`: 1 023, 1 024, 1 025 and 2 049 chunks.  One ungrouped batch: a seeded draw of bins plus the
    first and last bin of the range and of the chunks around the step, some of them repeated; expected from np.unique."""
    import torch

    from tracs_amd import device as dev
    rng = np.random.default_rng(1024)
    edges = [0, n_bins - 1] + [b for c in (1022, 1023, 1024, 1025) for b in (c * 1024, c * 1024 + 1023)]
    edges = [b for b in edges if b < n_bins]
    values = np.concatenate([rng.integers(0, n_bins, 3000), edges, edges[::2], rng.integers(0, n_bins, 50).repeat(3)]).astype(np.int64)
    rng.shuffle(values)
    assert (n_bins + 1023) // 1024 in (1023, 1024, 1025, 2049) and values.max() == n_bins - 1 and values.min() == 0
    uniq, counts = np.unique(values, return_counts=True)
    assert counts.max() >= 3 and len(uniq) > 3000
    zeros = np.zeros(len(uniq), np.uint64)
    val = torch.from_numpy(values.astype(np.int32)).cuda()
    state = dev.hist_init(n_bins)
    dev.hist_update_coo(state, n_bins, torch.zeros_like(val), torch.ones_like(val), val)
    check(emitted(state, n_bins), [uniq.astype(np.uint64), zeros, zeros, counts.astype(np.uint64)], ("scan seam", n_bins))


def test_histogram_ties(hiplib, oracle, tmp_path):
    n, L = 200, 3000
    same = np.repeat(seqs_for(1, L, seed=4, p_n=0.0, p_partial=0.0), n, axis=0)
    lab = random_labels(n, seed=2)
    h = histogram(tmp_path, same, lab)["snp"]
    check(h, expected(oracle, same, lab)[0], "all identical")
    assert h["value"].tolist() == [0] and int(h["within"][0] + h["between"][0] + h["ungrouped"][0]) == n * (n - 1) // 2
    check(histogram(tmp_path, same)["snp"], expected(oracle, same)[0], "all identical, no groups")
    seqs = seqs_for(n, L, seed=5, n_lineages=4)
    for g in range(0, n, 20):                              # blocks of identical sequences
        seqs[g + 1:g + 12] = seqs[g]
    for labels in (None, lab):
        check(histogram(tmp_path, seqs, labels)["snp"], expected(oracle, seqs, labels)[0], ("blocks", labels is not None))


def test_histogram_wide_range_takes_every_route(hiplib, oracle):
    """Two lineages ~10 % apart at L = 200 000, near-identical samples inside each: one panel holds d ~ 0 and d ~ 20 000.  The founders
    differ at a multiple of the kernel's LDS window, so both modes want the same slots: whichever claims a slot counts in LDS, the
    other takes the global route; a block of identical samples feeds the combined route."""
    import torch

    from tracs_amd import device as dev
    window = dev.hist_routes(dev.hist_init(1))["window"]
    L, per = 200000, 60
    rng = np.random.default_rng(41)
    bases = np.frombuffer(b"ACGT", np.uint8)
    a = rng.integers(0, 4, L)
    b = a.copy()
    sites = rng.choice(L, 20 * window, replace=False)              # 20 480 sites at a window of 1 024: ~10 % of L
    b[sites] = (b[sites] + rng.integers(1, 4, len(sites))) % 4
    rows = []
    for founder in (a, b):
        for _ in range(per):
            s = founder.copy()
            hit = rng.choice(L, rng.poisson(10), replace=False)
            s[hit] = (s[hit] + rng.integers(1, 4, len(hit))) % 4
            rows.append(s)
    seqs = bases[np.array(rows)]
    seqs[5:30] = seqs[4]                                          # identical samples: runs of one value in a row of the panel
    seqs[rng.random(seqs.shape) < 1e-4] = ord("N")
    lab = np.repeat(np.arange(2, dtype=np.int32), per)
    lab[rng.choice(2 * per, 6, replace=False)] = -1
    n = 2 * per
    _, _, d_all, _ = oracle.pairsnp_arrays(seqs, n_threads=8)
    assert d_all.min() == 0 and d_all.max() > 20000 and ((d_all > 100) & (d_all < 20000)).sum() == 0
    aln, d, _ = dense_panel(seqs)
    for labels in (lab, None):
        state = dev.hist_init(L + 1)
        dev.hist_update(state, L + 1, d, n, group=None if labels is None else torch.from_numpy(labels).cuda())
        check(emitted(state, L + 1), expected(oracle, seqs, labels)[0], ("wide", labels is not None))
        routes = dev.hist_routes(state)
        assert routes["combined"] > 0 and routes["lds"] > 0 and routes["global"] > 0, routes
        assert routes["combined"] + routes["lds"] + routes["global"] == n * (n - 1) // 2, routes
    aln.close()


def test_histogram_more_than_2_to_32_in_one_bin(hiplib):
    import torch

    from tracs_amd import device as dev
    n = 30000
    panel = torch.zeros((n, n), dtype=torch.int32, device="cuda")          # 3.6 GB, every pair at distance 0
    state = dev.hist_init(4)
    for _ in range(10):
        dev.hist_update(state, 4, panel, n)
    v, w, b, u = emitted(state, 4)
    assert v.tolist() == [0] and w.tolist() == [0] and b.tolist() == [0]
    assert u.tolist() == [10 * (n * (n - 1) // 2)] == [4499850000] and u[0] > 2 ** 32
    # with labels: the same total, split exactly
    lab = torch.arange(n, dtype=torch.int32, device="cuda") % 3
    state = dev.hist_init(4)
    for _ in range(10):
        dev.hist_update(state, 4, panel, n, group=lab)
    v, w, b, u = emitted(state, 4)
    within = 10 * 3 * (10000 * 9999 // 2)
    assert v.tolist() == [0] and w.tolist() == [within] and b.tolist() == [4499850000 - within] and u.tolist() == [0]
    del panel
    # a value >= n_bins is counted apart and makes the emit fail: nothing is dropped silently
    small = torch.tensor([[0, 1, 5], [0, 0, 2], [0, 0, 0]], dtype=torch.int32, device="cuda")
    state = dev.hist_init(3)
    dev.hist_update(state, 3, small, 3)
    with pytest.raises(RuntimeError, match="1 values were offered that are not below n_bins = 3"):
        dev.hist_emit(state, 3)
    state = dev.hist_init(6)
    dev.hist_update(state, 6, small, 3)
    v, w, b, u = emitted(state, 6)
    assert v.tolist() == [1, 2, 5] and u.tolist() == [1, 1, 1]


def test_histogram_filter(hiplib, oracle, tmp_path):
    seqs = seqs_for(90, 20000, seed=17, n_lineages=3)
    lab = random_labels(90, seed=8)
    _, _, d_all, _ = oracle.pairsnp_arrays(seqs, n_threads=8)
    for thr in (2147483647, int(np.percentile(d_all, 40))):
        r, c, d, _ = oracle.pairsnp_arrays(seqs, dist=thr, n_threads=8)
        filt = oracle.filter_recomb_pairs(seqs, r, c, n_threads=8)
        h = histogram(tmp_path, seqs, lab, dist=thr, filter=True)
        cls = classes_of(lab, r, c)
        check(h["snp"], bincount_hist(d, cls), ("filter: snp", thr))
        check(h["filter"], bincount_hist(filt, cls), ("filter: filter", thr))             # eligibility stays by the raw d
        assert int(sum(h["filter"][k].sum() for k in CLASSES)) == len(r)


def test_histogram_large_against_oracle(hiplib, oracle, tmp_path):
    """2 000 x 200 kbp with lineages and groups, through several row panels of the device primitives and through the library's own loop."""
    import torch

    from tracs_amd import device as dev
    n, L = 2000, 200000
    seqs = seqs_for(n, L, seed=23, n_lineages=40, mu_lineage=5e-4, mu_sample=5e-5, p_n=0.01, p_partial=0.0005)
    lab = random_labels(n, seed=23)
    exp, pairs = expected(oracle, seqs, lab)
    aln = dev.Alignment(n, L)
    aln.pack(seqs)
    state = dev.hist_init(L + 1)
    g = torch.from_numpy(lab).cuda()
    panel = 700
    d = torch.empty((panel, n), dtype=torch.int32, device="cuda")
    nn = torch.empty_like(d)
    for r0 in range(0, n, panel):
        r1 = min(n, r0 + panel)
        dev.pairsnp_dense(aln, d, nn, row_begin=r0, row_end=r1, dist_threshold=2147483647, base_row=r0)
        dev.hist_update(state, L + 1, d, n, row_begin=r0, row_end=r1, group=g, base_row=r0)
    got = emitted(state, L + 1)
    aln.close()
    check(got, exp, "2000 x 200 kbp, primitives")
    assert pairs == n * (n - 1) // 2
    check(histogram(tmp_path, seqs, lab)["snp"], exp, "2000 x 200 kbp, library")


def structured_alignment(rng, n_lineages=8, per_lineage=15, L=20000):
    """Lineages with mutation rates of their own (over-dispersed between-lineage distances); groups = lineage, a few strangers."""
    bases = np.frombuffer(b"ACGT", np.uint8)
    anc = rng.integers(0, 4, L)

    def mutate(code, rate):
        out = code.copy()
        hit = rng.random(L) < rate
        out[hit] = (out[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        return out
    rows, lab = [], []
    for g in range(n_lineages):
        founder = mutate(anc, rng.uniform(2e-3, 1.5e-2))
        for _ in range(per_lineage):
            rows.append(mutate(founder, 2e-4))
            lab.append(g)
    lab = np.array(lab, np.int32)
    s = rng.choice(len(lab), 2 * n_lineages, replace=False)
    lab[s] = (lab[s] + rng.integers(1, n_lineages, len(s))) % n_lineages
    lab[rng.choice(len(lab), 5, replace=False)] = -1
    return bases[np.array(rows)], lab


def test_histogram_cli_then_threshold(hiplib, oracle, tmp_path):
    from tracs_amd import synth
    from tracs_amd import threshold as th
    seqs, lab = structured_alignment(np.random.default_rng(77))
    n = len(lab)
    names = ["iso%d" % i for i in range(n)]
    fa = str(tmp_path / "refX_combined.fasta")
    synth.write_fasta(fa, seqs, names=names)
    gp = str(tmp_path / "groups.csv")
    with open(gp, "w") as fh:
        fh.write("sample,group\n")
        for nm, g in zip(names, lab):
            fh.write("%s,%s\n" % (nm, ("lineage%d" % g) if g >= 0 else ""))
        fh.write("not_in_the_alignment,lineage0\n")
    hist = str(tmp_path / "hist.csv")
    p = subprocess.run([sys.executable, "-m", "tracs_amd", "distance", "--msa", fa, "-o", hist, "--histogram", "--groups", gp, "--filter",
                        "--loglevel", "ERROR"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    r, c, d, _ = oracle.pairsnp_arrays(seqs, n_threads=8)
    filt = oracle.filter_recomb_pairs(seqs, r, c, n_threads=8)
    cls = classes_of(lab, r, c)
    want = ["column,distance,within,between,ungrouped,MSA file"]
    for column, values in (("snp", d), ("filter", filt)):
        v, w, b, u = bincount_hist(values, cls)
        want += ["%s,%d,%d,%d,%d,refX" % (column, a, x, y, z) for a, x, y, z in zip(v, w, b, u)]
    assert open(hist).read().split("\n") == want + [""]                       # row for row
    out = str(tmp_path / "threshold.csv")
    p = subprocess.run([sys.executable, "-m", "tracs_amd", "threshold", "--histogram", hist, "-o", out], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    got = dict(ln.split(",") for ln in open(out).read().strip().split("\n")[1:])

    def counts(x):
        v, k = np.unique(np.asarray(x).astype(np.int64), return_counts=True)
        return dict(zip(v.tolist(), k.tolist()))
    exp = th.fit(counts(d[cls == 0]), counts(d[cls == 1]))                  # the same fit on the oracle's pair lists
    assert exp["converged"] and got["converged"] == "True"
    assert float(got["snp_threshold"]) == exp["snp_threshold"] and exp["snp_threshold"] > 0
    for k in ("r", "p", "q", "lambda"):
        assert abs(float(got[k]) - exp[k]) <= 1e-4, (k, got[k], exp[k])
    assert int(got["n_close"]) == int((cls == 0).sum()) and int(got["n_distant"]) == int((cls == 1).sum())
    assert "SNP threshold" in p.stderr
