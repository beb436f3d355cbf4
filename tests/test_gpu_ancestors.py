"""Each sample's most likely earlier source (tracs_anc_*: csrc/ancestors.hip; tracs_distance_ancestors; `distance --ancestors WEIGHT`)
against the definition (tests/ancestors_ref.py) over random dated graphs or the full run's rows.  Every comparison is exact."""
import argparse
import os
import subprocess
import sys
from datetime import date, timedelta

import numpy as np
import pytest

import ancestors_ref as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL = {"snp": 3, "filter": 6, "direct": 4, "expectedK": 5}
KIND = {"snp": 0, "filter": 0, "direct": 2, "expectedK": 1}
HEADER = "sampleA,sampleB,date difference,SNP distance,transmission distance,expected K,filtered SNP distance,sites considered,MSA file\n"
TREE_HEADER = "sample,date,ancestor,ancestor date,root,generation,MSA file\n"
POOL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-300, 0.25, 0.25, 3.0])      # the forest test's pool


# ---- the device primitives ------------------------------------------------------------------------------------------------

def _run(n, days, i, j, v, kind, batches, e_mask=None, e_max=-1.0):
    """The pairs offered in `batches` (index arrays) -> (candidates offered, links, parent, root, generation) as numpy arrays.  Every
    pair carries its position as d, 7 x it as nn and position + 0.5 as p, so that the gathered values identify the chosen pair."""
    import torch

    from tracs_amd import device as dev
    m = len(i)
    ids = np.arange(m, dtype=np.int32)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    state = dev.anc_init(n, cu(np.asarray(days, np.int32)))
    taken = 0
    for sl in batches:
        val = cu(np.asarray(v)[sl].astype(np.float64)) if kind else cu(np.asarray(v)[sl].astype(np.uint32).view(np.int32))
        taken += dev.anc_update(state, n, cu(np.asarray(i)[sl].astype(np.uint32).view(np.int32)), cu(np.asarray(j)[sl].astype(np.uint32).view(np.int32)),
                                val, descending=kind == 2, e_mask=None if e_mask is None else cu(e_mask[sl]), e_max=e_max, d=cu(ids[sl]),
                                nn=cu((ids[sl] * 7).astype(np.int32)), p=cu(np.arange(m, dtype=np.float64)[sl] + 0.5),
                                e=None if e_mask is None else cu(e_mask[sl]))
    return taken, [t.cpu().numpy() for t in dev.anc_emit(state, n)]


def _check(n, days, i, j, v, kind, e_mask=None, e_max=-1.0, n_batches=7):
    """One batch, n_batches batches and the same reversed: identical to each other and to the helper."""
    days = np.asarray(days, np.int64)
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    m = len(i)
    elig = None if e_mask is None else e_max >= e_mask                      # (a NaN fails)
    parent, edge = ar.ancestors(n, days, i, j, v, kind, elig)
    root, gen = ar.trees(parent)
    e_pos, lo, hi = ar.links(parent, edge)
    inside = (i != j) & (i < n) & (j < n)
    cand = inside & (days[np.where(inside, i, 0)] != days[np.where(inside, j, 0)]) & (True if elig is None else elig)
    chunks = np.array_split(np.arange(m), n_batches)
    ref = None
    for batches in ([np.arange(m)], chunks, chunks[::-1]):
        taken, (r, c, d, nn, filt, p, e, pa, ro, ge) = _run(n, days, i, j, v, kind, batches, e_mask, e_max)
        assert taken == int(cand.sum())
        assert np.array_equal(pa.astype(np.int64), parent)                 # (0xFFFFFFFF reads as -1)
        assert np.array_equal(ro.astype(np.int64), root) and np.array_equal(ge.astype(np.int64), gen)
        assert np.array_equal(r.astype(np.int64), lo) and np.array_equal(c.astype(np.int64), hi)
        assert np.array_equal(d.astype(np.int64), e_pos)
        assert np.array_equal(nn.astype(np.int64), e_pos * 7) and np.array_equal(p, e_pos + 0.5)
        assert not filt.any()
        assert (not e.any()) if e_mask is None else np.array_equal(e, e_mask[e_pos])
        got = [r, c, d, pa, ro, ge]
        assert ref is None or all(np.array_equal(x, y) for x, y in zip(got, ref))
        ref = got
    return parent, gen


def _graph(rng, n, m):
    a = rng.integers(0, n, m * 2)
    b = rng.integers(0, n, m * 2)
    keep = a != b
    lo, hi = np.minimum(a[keep], b[keep]), np.maximum(a[keep], b[keep])
    key = np.unique(lo.astype(np.int64) * n + hi)[:m]
    rng.shuffle(key)
    lo, hi = key // n, key % n
    flip = rng.random(len(lo)) < 0.5                      # either endpoint order
    return np.where(flip, hi, lo), np.where(flip, lo, hi)


def _days(rng, n, pool=9):
    return (rng.integers(0, pool, n) - pool // 2) * 3     # a small pool around 1970-01-01: many equal days and gaps, negative days


def test_anc_two_samples(hiplib):
    parent, _ = _check(2, [4, -3], [0], [1], [2], 0, n_batches=1)
    assert parent.tolist() == [1, -1]


def test_anc_all_days_equal(hiplib):
    rng = np.random.default_rng(1)
    i, j = _graph(rng, 30, 80)
    parent, gen = _check(30, np.full(30, -7), i, j, rng.integers(0, 4, len(i)), 0)
    assert (parent == -1).all() and (gen == 0).all()


@pytest.mark.parametrize("n,m,kind", [(50, 120, 0), (20, 63, 0), (20, 64, 1), (20, 65, 2), (3000, 30000, 1), (3000, 30000, 2),
                                      (70000, 200000, 0)])
def test_anc_primitives_against_the_definition(hiplib, n, m, kind):
    rng = np.random.default_rng(n + m + kind)
    i, j = _graph(rng, n, m)
    m = len(i)
    if kind == 0:
        v = rng.integers(0, 4, m)                         # heavy ties: the gap and the index decide
    else:
        v = np.where(rng.random(m) < 0.5, POOL[rng.integers(0, len(POOL), m)], rng.integers(0, 3, m) * 0.5)
    parent, _ = _check(n, _days(rng, n), i, j, v, kind)
    assert (parent >= 0).sum() > 0 and (n < 65536 or parent.max() >= 65536)


def test_anc_u32_values_above_2_31(hiplib):
    rng = np.random.default_rng(9)
    i, j = _graph(rng, 200, 2000)
    v = rng.integers(0, 2 ** 32, len(i), dtype=np.uint64)
    v[:40] = 2 ** 32 - 1
    _check(200, _days(rng, 200), i, j, v, 0)


def test_anc_extreme_days(hiplib):
    """Gaps up to 2^32 - 1: the gap is computed in 64 bits."""
    rng = np.random.default_rng(4)
    n = 40
    i, j = _graph(rng, n, 300)
    days = rng.choice(np.array([-2 ** 31, -2 ** 31 + 1, -1, 0, 1, 2 ** 31 - 2, 2 ** 31 - 1]), n)
    _check(n, days, i, j, np.zeros(len(i), np.int64), 0)


def test_anc_skips_loops_and_outside_endpoints(hiplib):
    rng = np.random.default_rng(6)
    n = 60
    i, j = _graph(rng, n, 400)
    i[::11] = j[::11]                                     # loops
    j[5::13] = n + rng.integers(0, 5, len(j[5::13]))      # endpoints >= n
    i[7::17] = 0xFFFFFFFF
    _check(n, _days(rng, n), i, j, rng.integers(0, 3, len(i)), 0)


@pytest.mark.parametrize("kind", [0, 2])
def test_anc_eligibility_mask(hiplib, kind):
    """e_mask / e_max: the -K test, a NaN fails it; skipped pairs are not counted as offered."""
    rng = np.random.default_rng(5)
    n = 400
    i, j = _graph(rng, n, 3000)
    ek = rng.normal(size=len(i)) * 3
    ek[::17] = np.nan
    v = rng.integers(0, 3, len(i)) if kind == 0 else rng.integers(0, 3, len(i)) * 0.25
    _check(n, _days(rng, n), i, j, v, kind, e_mask=ek, e_max=1.0)


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 2, 1, 0), (1, 0, 3, 2), (2, 3, 0, 1)])
def test_anc_cross_batch_by_hand(hiplib, order):
    """A later batch that lowers a sample's value discards the tie key kept so far; one that ties it competes with it."""
    import torch

    from tracs_amd import device as dev
    s, a1, a2 = 9, 1, 2
    days = np.array([0, 9, 1, 0, 5, 0, 0, 5, 0, 10], np.int32)            # s on day 10; a1: gap 1; a2: gap 9; 4 and 7: gap 5
    batches = [([s], [a1], [5]),                          # value 5, gap 1
               ([a2], [s], [3]),                          # value 3, gap 9: the value decides, whatever the gap
               ([s], [7], [3]),                           # value 3, gap 5: beats a2 on the gap
               ([4], [s], [3])]                           # value 3, gap 5, index 4: beats 7 on the index
    cu = lambda x, t: torch.from_numpy(np.asarray(x, t)).cuda()
    state = dev.anc_init(10, cu(days, np.int32))
    best = None
    rank = {a1: 3, a2: 2, 7: 1, 4: 0}                     # the order the definition puts s's candidates in
    for k in order:
        r, c, v = batches[k]
        assert dev.anc_update(state, 10, cu(r, np.int32), cu(c, np.int32), cu(v, np.int32), d=cu([100 + k], np.int32)) == 1
        a = c[0] if r[0] == s else r[0]
        best = (a, k) if best is None or rank[a] < rank[best[0]] else best
        rr, cc, d, _, _, _, _, pa, ro, ge = [t.cpu().numpy() for t in dev.anc_emit(state, 10)]
        assert pa[s] == best[0] and d.tolist() == [100 + best[1]]
        assert (rr.tolist(), cc.tolist()) == ([best[0]], [s]) and ro[s] == best[0] and ge[s] == 1
        assert (np.delete(pa, s) == -1).all()
    assert best[0] == 4


def test_anc_chain(hiplib):
    """5 000 samples, each linked to the one a day before it: generations 0 .. 4 999 under one root (pointer doubling)."""
    n = 5000
    rng = np.random.default_rng(2)
    perm = rng.permutation(n)                             # vertex perm[k] is sampled on day k - 2500
    days = np.empty(n, np.int64)
    days[perm] = np.arange(n) - 2500
    i, j = perm[:-1].copy(), perm[1:].copy()
    flip = rng.random(n - 1) < 0.5
    i[flip], j[flip] = perm[1:][flip], perm[:-1][flip]
    parent, gen = _check(n, days, i, j, rng.integers(0, 2, n - 1), 0)
    assert np.array_equal(gen[perm], np.arange(n)) and (parent >= 0).sum() == n - 1


def test_anc_star(hiplib):
    n = 300
    days = np.full(n, 3)
    days[17] = -2
    others = np.delete(np.arange(n), 17)
    parent, gen = _check(n, days, others, np.full(n - 1, 17), np.arange(n - 1) % 5 * 0.5, 2)
    assert (parent[others] == 17).all() and parent[17] == -1 and gen.max() == 1


def test_anc_rejects_bad_arguments(hiplib):
    import torch

    from tracs_amd import _lib
    from tracs_amd import device as dev
    days = torch.zeros(4, dtype=torch.int32, device="cuda")
    state = dev.anc_init(4, days)
    z = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="another vertex count"):
        dev.anc_update(state, 5, z, z, z)
    with pytest.raises(RuntimeError, match="value_kind"):
        _lib.check(hiplib.tracs_anc_update_coo(state.data_ptr(), 4, 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), 3, None, -1.0, None, None,
                                               None, None, None, None, None))


# ---- the CLI end to end -------------------------------------------------------------------------------------------------------

N, LEN = 97, 4000


def run_cli(argv):
    from tracs_amd.distance import distance_parser
    a = distance_parser(argparse.ArgumentParser()).parse_args(argv + ["--loglevel", "ERROR"])
    a.func(a)


def read_rows(path):
    text = open(path).read()
    assert text.startswith(HEADER)
    return [ln for ln in text[len(HEADER):].split("\n") if ln]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """97 x 4 000 with four lineages and a group of identical records, dates over 12 distinct days on both sides of 1970-01-01."""
    from tracs_amd import synth
    tmp = tmp_path_factory.mktemp("anc")
    seqs = synth.alignment(N, LEN, seed=41, mu_lineage=2e-3, mu_sample=5e-4, n_lineages=4, p_n=0.02, p_partial=0.005)
    seqs[10:14] = seqs[9]
    names = ["iso%d" % k for k in range(N)]
    fa = str(tmp / "refA_combined.fasta")
    synth.write_fasta(fa, seqs, names=names)
    rng = np.random.default_rng(41)
    slot = rng.integers(0, 12, N)
    assert len(set(slot.tolist())) == 12
    iso = [(date(1969, 12, 16) + timedelta(days=int(3 * k))).isoformat() for k in slot]
    days = np.array([(date.fromisoformat(x) - date(1970, 1, 1)).days for x in iso])
    assert days.min() < 0 < days.max()
    meta = str(tmp / "meta.csv")
    with open(meta, "w") as fh:
        fh.write("sample,date\n")
        for nm, x in zip(names, iso):
            fh.write("%s,%s\n" % (nm, x))
    return dict(tmp=tmp, seqs=seqs, names=names, fa=fa, iso=iso, days=days, meta=meta,
                common=["--msa", fa, "--meta", meta, "--clock_rate", "5.3", "--trans_rate", "6.0"])


def _value(field, weight):
    return int(field) if KIND[weight] == 0 else float(field)


def expected(frows, names, days, iso, weight, ref, kept=None):
    """The definition applied to the full run's rows -> (output lines, tree file text, parent).  kept: the compared samples (all)."""
    idx = {nm: k for k, nm in enumerate(names)}
    f = [r.split(",") for r in frows]
    i = np.array([idx[x[0]] for x in f], np.int64)
    j = np.array([idx[x[1]] for x in f], np.int64)
    v = np.array([_value(x[COL[weight]], weight) for x in f], np.int64 if KIND[weight] == 0 else np.float64)
    assert (i < j).all()
    parent, edge = ar.ancestors(len(names), days, i, j, v, KIND[weight])
    root, gen = ar.trees(parent)
    e_pos, lo, hi = ar.links(parent, edge)
    assert np.array_equal(i[e_pos], lo) and np.array_equal(j[e_pos], hi)
    tree = TREE_HEADER
    for s in (range(len(names)) if kept is None else kept):
        a = parent[s]
        tree += "%s,%s,%s,%s,%s,%d,%s\n" % (names[s], iso[s], names[a] if a >= 0 else "", iso[a] if a >= 0 else "", names[root[s]], gen[s], ref)
    return [frows[k] for k in e_pos], tree, parent


def _cli_child(argv, env):
    p = subprocess.run([sys.executable, "-m", "tracs_amd", "distance"] + argv + ["--loglevel", "ERROR"], capture_output=True, text=True,
                       env=dict(os.environ, **env), timeout=300, cwd=ROOT)
    assert p.returncode == 0, (env, p.stdout[-1500:] + p.stderr[-3000:])


@pytest.mark.parametrize("weight", ["snp", "filter", "direct", "expectedK"])
def test_ancestors_cli_rows_and_trees(hiplib, case, weight):
    tmp = case["tmp"]
    common = case["common"] + (["--filter"] if weight == "filter" else [])
    full, out, tree = str(tmp / ("full_%s.csv" % weight)), str(tmp / ("anc_%s.csv" % weight)), str(tmp / ("tree_%s.csv" % weight))
    run_cli(common + ["-o", full])
    frows = read_rows(full)
    assert len(frows) == N * (N - 1) // 2
    lines, tree_text, parent = expected(frows, case["names"], case["days"], case["iso"], weight, "refA")
    assert 0 < len(lines) <= N - 1 and (parent[case["days"] == case["days"].min()] == -1).all()
    run_cli(common + ["-o", out, "--ancestors", weight, "--ancestors-out", tree])
    assert open(out).read() == HEADER + "".join(ln + "\n" for ln in lines)
    assert open(tree).read() == tree_text
    # the same bytes when every link crosses panel boundaries (the panel height is read once per process: a child)
    _cli_child(common + ["-o", out + ".p7", "--ancestors", weight, "--ancestors-out", tree + ".p7"], {"TRACS_FOREST_PANEL_ROWS": "7"})
    assert open(out + ".p7").read() == open(out).read() and open(tree + ".p7").read() == tree_text


def test_ancestors_cli_thresholds_leave_samples_without_a_candidate(hiplib, case):
    tmp = case["tmp"]
    full0 = str(tmp / "t_full0.csv")
    run_cli(case["common"] + ["-o", full0])
    f0 = [r.split(",") for r in read_rows(full0)]
    thr = int(np.percentile([int(x[3]) for x in f0], 20))
    kmax = max(1, int(np.nanpercentile([float(x[5]) for x in f0], 40)))
    _, _, parent0 = expected(read_rows(full0), case["names"], case["days"], case["iso"], "expectedK", "refA")
    extra = ["-D", str(thr), "-K", str(kmax)]
    full, out, tree = str(tmp / "t_full.csv"), str(tmp / "t_anc.csv"), str(tmp / "t_tree.csv")
    run_cli(case["common"] + extra + ["-o", full])
    frows = read_rows(full)
    assert 0 < len(frows) < len(f0)
    lines, tree_text, parent = expected(frows, case["names"], case["days"], case["iso"], "expectedK", "refA")
    assert (parent == -1).sum() > (parent0 == -1).sum() and len(lines) > 0        # some samples lost every candidate
    run_cli(case["common"] + extra + ["-o", out, "--ancestors", "expectedK", "--ancestors-out", tree])
    assert open(out).read() == HEADER + "".join(ln + "\n" for ln in lines)
    assert open(tree).read() == tree_text


def test_ancestors_cli_sample_and_pair_rules(hiplib, case, tmp_path):
    """A planted low-coverage sample without a date: the sample rule leaves it out before dates are looked up; --min-sites removes
    pairs; --msa-out and --site-table still work on this route."""
    from tracs_amd import synth
    seqs = case["seqs"].copy()
    low = 40
    rng = np.random.default_rng(8)
    seqs[low, rng.random(LEN) < 0.6] = ord("N")
    fa = str(tmp_path / "refB_combined.fasta")
    synth.write_fasta(fa, seqs, names=case["names"])
    meta = str(tmp_path / "meta.csv")
    with open(meta, "w") as fh:
        fh.write("sample,date\n")
        for k, (nm, x) in enumerate(zip(case["names"], case["iso"])):
            if k != low:
                fh.write("%s,%s\n" % (nm, x))
    base = ["--msa", fa, "--meta", meta, "--clock_rate", "5.3", "--trans_rate", "6.0", "--max-sample-n-share", "0.3"]
    probe = str(tmp_path / "probe.csv")
    run_cli(base + ["-o", probe])
    sites = np.array([int(r.split(",")[7]) for r in read_rows(probe)])
    rules = base + ["--min-sites", str(int(np.median(sites)))]
    full, out, tree = str(tmp_path / "full.csv"), str(tmp_path / "anc.csv"), str(tmp_path / "tree.csv")
    run_cli(rules + ["-o", full])
    frows = read_rows(full)
    assert 0 < len(frows) < len(sites)
    kept = [k for k in range(N) if k != low]
    lines, tree_text, _ = expected(frows, case["names"], case["days"], case["iso"], "snp", "refB", kept=kept)
    msa_out, table = str(tmp_path / "cmp.fa"), str(tmp_path / "sites.csv")
    run_cli(rules + ["-o", out, "--ancestors", "snp", "--ancestors-out", tree, "--msa-out", msa_out, "--site-table", table])
    assert open(out).read() == HEADER + "".join(ln + "\n" for ln in lines) and len(lines) > 0
    assert open(tree).read() == tree_text
    gone = case["names"][low]
    assert all(gone not in ln.split(",") for ln in open(out).read().split("\n") + open(tree).read().split("\n"))
    assert open(msa_out).read().count(">") == N - 1 and os.path.getsize(table) > 0


def test_ancestors_missing_date_names_the_sample(hiplib, case, tmp_path):
    meta = str(tmp_path / "meta.csv")
    with open(meta, "w") as fh:
        fh.write("sample,date\n")
        for nm, x in list(zip(case["names"], case["iso"]))[:-1]:
            fh.write("%s,%s\n" % (nm, x))
    with pytest.raises(SystemExit) as e:
        run_cli(["--msa", case["fa"], "--meta", meta, "-o", str(tmp_path / "o.csv"), "--ancestors", "snp"])
    assert case["names"][-1] in str(e.value.code) and "--ancestors" in str(e.value.code)


def test_ancestors_two_msa_files_append(hiplib, case, tmp_path):
    from tracs_amd import synth
    fb = str(tmp_path / "refC_combined.fasta")
    synth.write_fasta(fb, case["seqs"][::-1][:30], names=case["names"][:30])
    out, tree = str(tmp_path / "anc.csv"), str(tmp_path / "tree.csv")
    run_cli(["--msa", case["fa"], fb, "--meta", case["meta"], "-o", out, "--ancestors", "snp", "--ancestors-out", tree])
    want, want_tree = HEADER, TREE_HEADER
    for fa, names, ref in ((case["fa"], case["names"], "refA"), (fb, case["names"][:30], "refC")):
        full = str(tmp_path / ("full_%s.csv" % ref))
        run_cli(["--msa", fa, "--meta", case["meta"], "-o", full])
        lines, tree_text, _ = expected(read_rows(full), names, case["days"][:len(names)], case["iso"][:len(names)], "snp", ref)
        want += "".join(ln + "\n" for ln in lines)
        want_tree += tree_text[len(TREE_HEADER):]
    assert open(out).read() == want and open(tree).read() == want_tree
