"""Minimum spanning forest of the eligible pairs (tracs_msf_*: csrc/forest.hip; tracs_distance_forest; `distance --mst WEIGHT`)
against Kruskal under (weight, i, j) (tests/forest_ref.py) over the oracle's pairs or the full run's rows.  Every comparison is exact."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

import forest_ref as fr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL = {"snp": 3, "filter": 6, "direct": 4, "expectedK": 5}


def seqs_for(n, L, seed, **kw):
    from tracs_amd import synth
    args = dict(mu_lineage=3e-3, mu_sample=1e-3, p_n=0.02, p_partial=0.005)
    args.update(kw)
    return synth.alignment(n, L, seed=seed, **args)


def write(path, seqs, prefix="s"):
    from tracs_amd import synth
    names = ["%s%d" % (prefix, i) for i in range(seqs.shape[0])]
    synth.write_fasta(str(path), seqs, names=names)
    return names


def run_cli(argv):
    from tracs_amd.distance import distance_parser
    a = distance_parser(argparse.ArgumentParser()).parse_args(argv + ["--loglevel", "ERROR"])
    a.func(a)


def read_rows(path):
    lines = open(path).read().split("\n")
    assert lines[0] + "\n" == "sampleA,sampleB,date difference,SNP distance,transmission distance,expected K,filtered SNP distance," \
                              "sites considered,MSA file\n"
    return [ln for ln in lines[1:] if ln]


def check_rows(rows, names, exp, what):
    """rows of a forest file against (rows, cols, d, nn) expected in (i, j) order."""
    idx = {nm: i for i, nm in enumerate(names)}
    got = np.array([[idx[f[0]], idx[f[1]], int(f[3]), int(f[7])] for f in (r.split(",") for r in rows)], np.int64).reshape(-1, 4)
    e = np.stack([np.asarray(x, np.int64) for x in exp], axis=1).reshape(-1, 4)
    assert got.shape == e.shape, (what, got.shape, e.shape)
    assert np.array_equal(got, e), (what, np.flatnonzero((got != e).any(axis=1))[:5])


def oracle_forest(O, seqs, n0=None, dist=2147483647):
    r, c, d, nn = O.pairsnp_arrays(seqs, n0=n0, dist=dist, n_threads=8)
    f = fr.forest(seqs.shape[0], r, c, d)
    return r[f], c[f], d[f], nn[f]


# ---- the device primitives ------------------------------------------------------------------------------------------------

def _prims(n, i, j, w, batches):
    import torch

    from tracs_amd import device as dev
    m = len(i)
    ids = np.arange(m, dtype=np.int32)
    wf = np.asarray(w)
    state = dev.msf_init(n)
    taken = 0
    for sl in batches:
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        wt = cu(wf[sl].astype(np.float64)) if wf.dtype.kind == "f" else cu(wf[sl].astype(np.uint32).view(np.int32))
        taken += dev.msf_update(state, n, cu(i[sl].astype(np.int32)), cu(j[sl].astype(np.int32)), wt, d=cu(ids[sl]),
                                nn=cu((ids[sl] * 7).astype(np.int32)), p=cu(np.arange(m, dtype=np.float64)[sl] + 0.5))
    assert taken == m
    return [t.cpu().numpy() for t in dev.msf_emit(state, n)]


def _graph(rng, n, m):
    a = rng.integers(0, n, m * 2)
    b = rng.integers(0, n, m * 2)
    keep = a != b
    lo, hi = np.minimum(a[keep], b[keep]), np.maximum(a[keep], b[keep])
    key = np.unique(lo.astype(np.int64) * n + hi)[:m]
    rng.shuffle(key)
    lo, hi = key // n, key % n
    flip = rng.random(len(lo)) < 0.5
    return np.where(flip, hi, lo), np.where(flip, lo, hi)


@pytest.mark.parametrize("n,m,kind", [(2, 1, "ties"), (50, 120, "ties"), (1000, 20000, "u32"), (3000, 30000, "f64"),
                                      (200000, 400000, "ties"), (5000, 4000, "f64")])
def test_msf_primitives_against_kruskal(hiplib, n, m, kind):
    rng = np.random.default_rng(n + m)
    i, j = _graph(rng, n, m)
    m = len(i)
    if kind == "ties":
        w = rng.integers(0, 4, m)
    elif kind == "u32":
        w = rng.integers(0, 2 ** 32, m, dtype=np.uint64)
        w[:50] = 2 ** 32 - 1
    else:
        pool = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-300, 0.25, 0.25, 3.0])
        w = np.where(rng.random(m) < 0.5, pool[rng.integers(0, len(pool), m)], rng.normal(size=m))
    f = fr.forest(n, i, j, w)
    chunks = np.array_split(np.arange(m), 7)
    ref = None
    for batches in ([np.arange(m)], chunks, chunks[::-1]):
        r, c, d, nn, filt, p, e = _prims(n, i, j, w, batches)
        assert np.array_equal(r.astype(np.int64), np.minimum(i, j)[f]) and np.array_equal(c.astype(np.int64), np.maximum(i, j)[f])
        assert np.array_equal(d.astype(np.int64), f), kind
        assert np.array_equal(nn.astype(np.int64), f * 7) and np.array_equal(p, f + 0.5)
        assert not filt.any() and not e.any()
        got = np.stack([r, c, d])
        assert ref is None or np.array_equal(got, ref)
        ref = got


def test_msf_eligibility_mask(hiplib):
    """e_mask / e_max: the -K test, a NaN fails it; skipped pairs are not counted as taken."""
    import torch

    from tracs_amd import device as dev
    rng = np.random.default_rng(5)
    n = 400
    i, j = _graph(rng, n, 3000)
    w = rng.integers(0, 3, len(i))
    ek = rng.normal(size=len(i)) * 3
    ek[::17] = np.nan
    ok = 1.0 >= ek
    state = dev.msf_init(n)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    taken = dev.msf_update(state, n, cu(i.astype(np.int32)), cu(j.astype(np.int32)), cu(w.astype(np.int32)), e_mask=cu(ek), e_max=1.0,
                           e=cu(ek))
    assert taken == int(ok.sum())
    r, c, _, _, _, _, e = [t.cpu().numpy() for t in dev.msf_emit(state, n)]
    sel = np.flatnonzero(ok)
    f = sel[fr.forest(n, i[sel], j[sel], w[sel])]
    assert np.array_equal(r.astype(np.int64), np.minimum(i, j)[f]) and np.array_equal(c.astype(np.int64), np.maximum(i, j)[f])
    assert np.array_equal(e, ek[f])


# ---- `distance --mst snp` against the oracle -----------------------------------------------------------------------------

SHAPES = [(2, 1), (5, 37), (65, 1000), (130, 4097), (300, 20000)]


@pytest.mark.parametrize("n,L", SHAPES, ids=lambda v: str(v))
def test_mst_snp_shapes(hiplib, oracle, tmp_path, n, L):
    seqs = seqs_for(n, L, seed=n * 31 + L, n_lineages=3)
    fa = tmp_path / "a.fa"
    names = write(fa, seqs)
    _, _, d_all, _ = oracle.pairsnp_arrays(seqs, n_threads=8)
    for thr in sorted({2147483647, max(1, int(np.percentile(d_all, 20))) if len(d_all) else 1}):
        out = str(tmp_path / "f.csv")
        run_cli(["--msa", str(fa), "-o", out, "--mst", "snp", "-D", str(thr)])
        rows = read_rows(out)
        check_rows(rows, names, oracle_forest(oracle, seqs, dist=thr), (n, L, thr))
        assert all(r.split(",")[2] == "NA" and r.split(",")[6] == "0" and r.endswith(",a") for r in rows)


def test_mst_identical_groups(hiplib, oracle, tmp_path):
    seqs = seqs_for(200, 3000, seed=5, n_lineages=4)
    for g in range(0, 200, 20):                       # groups of identical sequences: every weight of a group ties
        seqs[g + 1:g + 12] = seqs[g]
    fa = tmp_path / "t.fa"
    names = write(fa, seqs)
    out = str(tmp_path / "f.csv")
    for thr in (2147483647, 3):
        run_cli(["--msa", str(fa), "-o", out, "--mst", "snp", "-D", str(thr)])
        check_rows(read_rows(out), names, oracle_forest(oracle, seqs, dist=thr), ("ties", thr))


def test_mst_msa_db_and_two_files(hiplib, oracle, tmp_path):
    allseqs = seqs_for(170, 5000, seed=11, n_lineages=6)
    q, db = allseqs[:40], allseqs[40:]
    fq, fdb = tmp_path / "q.fa", tmp_path / "db.fa"
    qn = write(fq, q)
    dn = write(fdb, db, prefix="db")
    out = str(tmp_path / "f.csv")
    run_cli(["--msa", str(fq), "--msa-db", str(fdb), "-o", out, "--mst", "snp"])
    rows = read_rows(out)
    exp = oracle_forest(oracle, allseqs, n0=40)
    check_rows(rows, qn + dn, exp, "msa-db")
    assert (np.asarray(exp[0]) < 40).all() and (np.asarray(exp[1]) >= 40).all()
    # two --msa files: each file's forest appended in turn
    a, b = seqs_for(90, 4000, seed=21, n_lineages=3), seqs_for(60, 4000, seed=22, n_lineages=2)
    fa, fb = tmp_path / "A.fa", tmp_path / "B.fa"
    an, bn = write(fa, a), write(fb, b, prefix="b")
    run_cli(["--msa", str(fa), str(fb), "-o", out, "--mst", "snp"])
    rows = read_rows(out)
    ea, eb = oracle_forest(oracle, a), oracle_forest(oracle, b)
    check_rows(rows[:len(ea[0])], an, ea, "file A")
    check_rows(rows[len(ea[0]):], bn, eb, "file B")
    assert all(r.endswith(",A") for r in rows[:len(ea[0])]) and all(r.endswith(",B") for r in rows[len(ea[0]):])


def test_mst_no_eligible_pair(hiplib, tmp_path):
    rng = np.random.default_rng(3)
    seqs = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (6, 4000))]
    fa = tmp_path / "x.fa"
    write(fa, seqs)
    out = str(tmp_path / "f.csv")
    run_cli(["--msa", str(fa), "-o", out, "--mst", "snp", "-D", "1"])
    assert read_rows(out) == []


ROUTE_CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from tracs_amd import synth
from tracs_amd.__main__ import main
seqs = synth.alignment(120, 30000, seed=7, mu_lineage=2e-3, mu_sample=3e-4, n_lineages=4, p_n=0.02, p_partial=0.003, p_other=0.001)
seqs[30:36] = seqs[29]
synth.write_fasta(sys.argv[1] + ".fa", seqs, names=["s%%d" %% i for i in range(120)])
sys.argv = ["tracs_amd", "distance", "--msa", sys.argv[1] + ".fa", "-o", sys.argv[1] + ".csv", "--mst", "snp", "--loglevel", "ERROR"]
main()
'''

ROUTES = [{}, {"TRACS_SITE_CLASSES": "1"}, {"TRACS_SITE_CLASSES": "0"}, {"TRACS_MFMA": "0"}, {"TRACS_FOREST_PANEL_ROWS": "7"},
          {"TRACS_FOREST_PANEL_ROWS": "1", "TRACS_SITE_CLASSES": "0"}]


def test_mst_same_bytes_on_every_route_and_panel(hiplib, oracle, tmp_path):
    from tracs_amd import synth
    outs = []
    for k, env in enumerate(ROUTES):
        (tmp_path / ("r%d" % k)).mkdir()
        base = str(tmp_path / ("r%d" % k) / "aln")             # one file name: the MSA column comes from it
        p = subprocess.run([sys.executable, "-c", ROUTE_CHILD % {"root": ROOT}, base], capture_output=True, text=True,
                           env=dict(os.environ, **env), timeout=300, cwd=ROOT)
        assert p.returncode == 0, (env, p.stdout[-1500:] + p.stderr[-3000:])
        outs.append(open(base + ".csv", "rb").read())
    for env, o in zip(ROUTES, outs):
        assert o == outs[0], env
    seqs = synth.alignment(120, 30000, seed=7, mu_lineage=2e-3, mu_sample=3e-4, n_lineages=4, p_n=0.02, p_partial=0.003, p_other=0.001)
    seqs[30:36] = seqs[29]
    rows = [r for r in outs[0].decode().split("\n")[1:] if r]
    check_rows(rows, ["s%d" % i for i in range(120)], oracle_forest(oracle, seqs), "routes")


# ---- the CLI end to end with --meta: byte-identical rows, the same clusters -------------------------------------------------

def _weight_of(row, weight):
    f = row.split(",")
    return float(f[COL[weight]])


def _clusters(path, weight, t, tmp_path):
    from tracs_amd import cluster as cl
    cl._ids.clear()                                    # the id table persists across calls in one process (tracs/cluster.py)
    out = str(tmp_path / "cl.csv")
    if os.path.exists(out):
        os.remove(out)
    a = cl.cluster_parser(argparse.ArgumentParser()).parse_args(["-d", path, "-o", out, "-c", repr(float(t)), "-D", weight,
                                                                 "--loglevel", "ERROR"])
    a.func(a)
    if not os.path.exists(out):
        return None
    groups = {}
    for ln in open(out).read().split("\n")[1:]:
        if ln:
            nm, lab = ln.rsplit(",", 1)
            groups.setdefault(lab, set()).add(nm)
    return {frozenset(g) for g in groups.values()}


@pytest.mark.parametrize("weight", ["snp", "filter", "direct", "expectedK"])
def test_mst_cli_meta_rows_and_clusters(hiplib, tmp_path, weight):
    from tracs_amd import synth
    n, L = 70, 20000
    seqs = seqs_for(n, L, seed=29, n_lineages=4, mu_lineage=2e-4, mu_sample=1e-4)
    seqs[10:14] = seqs[9]
    fa = tmp_path / "refX_combined.fasta"
    names = write(fa, seqs, prefix="iso")
    iso, _ = synth.dates(n, seed=29)
    meta = str(tmp_path / "meta.csv")
    with open(meta, "w") as fh:
        fh.write("sample,date\n")
        for nm, s in zip(names, iso):
            fh.write("%s,%s\n" % (nm, s))
    common = ["--msa", str(fa), "--meta", meta, "--clock_rate", "5.3", "--trans_rate", "6.0"] + (["--filter"] if weight == "filter" else [])
    full0 = str(tmp_path / "full0.csv")
    run_cli(common + ["-o", full0])
    ek = np.array([_weight_of(r, "expectedK") for r in read_rows(full0)])
    kmax = max(1, int(np.nanpercentile(ek, 40)))
    idx = {nm: i for i, nm in enumerate(names)}
    for extra in ([], ["-K", str(kmax)]):
        full, mst = str(tmp_path / "full.csv"), str(tmp_path / "mst.csv")
        run_cli(common + extra + ["-o", full])
        run_cli(common + extra + ["-o", mst, "--mst", weight])
        frows, mrows = read_rows(full), read_rows(mst)
        assert len(frows) > len(mrows) > 0
        i = np.array([idx[r.split(",")[0]] for r in frows])
        j = np.array([idx[r.split(",")[1]] for r in frows])
        w = np.array([_weight_of(r, weight) for r in frows])
        f = fr.forest(n, i, j, w)
        assert mrows == [frows[k] for k in f], (weight, extra)
        vals = np.unique(w[~np.isnan(w)])
        pick = vals[np.linspace(0, len(vals) - 1, min(len(vals), 6)).astype(int)]
        ts = sorted({0.0, float(vals.max()) + 1.0} | set(pick.tolist())
                    | {float((a + b) / 2) for a, b in zip(pick[:-1], pick[1:])})
        assert len(ts) >= 10 or len(vals) < 5
        for t in ts:
            assert _clusters(mst, weight, t, tmp_path) == _clusters(full, weight, t, tmp_path), (weight, extra, t)


def test_mst_missing_date_names_the_sample(hiplib, tmp_path):
    seqs = seqs_for(12, 3000, seed=3)
    fa = tmp_path / "m.fa"
    names = write(fa, seqs)
    meta = str(tmp_path / "meta.csv")
    with open(meta, "w") as fh:
        fh.write("sample,date\n")
        for nm in names[:-1]:
            fh.write("%s,2020-01-01\n" % nm)
    with pytest.raises(SystemExit) as e:
        run_cli(["--msa", str(fa), "--meta", meta, "-o", str(tmp_path / "o.csv"), "--mst", "snp"])
    assert names[-1] in str(e.value.code)


SIZE_CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from tracs_amd import synth
from tracs_amd.__main__ import main
seqs = synth.alignment(2000, 200000, seed=23, n_lineages=40, mu_lineage=5e-4, mu_sample=5e-5, p_n=0.01, p_partial=0.0005)
synth.write_fasta(sys.argv[1] + ".fa", seqs, names=["s%%d" %% i for i in range(2000)])
sys.argv = ["tracs_amd", "distance", "--msa", sys.argv[1] + ".fa", "-o", sys.argv[1] + ".csv", "--mst", "snp", "--loglevel", "ERROR"]
main()
'''


def test_mst_large_against_oracle(hiplib, oracle, tmp_path):
    """~2 000 x 200 kbp with lineages, through three row panels."""
    from tracs_amd import synth
    base = str(tmp_path / "big")
    p = subprocess.run([sys.executable, "-c", SIZE_CHILD % {"root": ROOT}, base], capture_output=True, text=True,
                       env=dict(os.environ, TRACS_FOREST_PANEL_ROWS="700"), timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    seqs = synth.alignment(2000, 200000, seed=23, n_lineages=40, mu_lineage=5e-4, mu_sample=5e-5, p_n=0.01, p_partial=0.0005)
    rows = read_rows(base + ".csv")
    assert len(rows) == 1999
    check_rows(rows, ["s%d" % i for i in range(2000)], oracle_forest(oracle, seqs), "2000 x 200 kbp")
