"""`tracs distance` under the sample rule and the pair rule, through the FASTA entry points and the command line.
--max-sample-n-share: the run writes, byte for byte, what the ordinary run writes on the FASTA with the dropped records (and, with site
rules, the dropped columns) deleted.  --min-sites: the ordinary run's rows without those compared over fewer sites, for the full
output, --nearest, --mst and --histogram."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import forest_ref as fr
from sample_rules_common import F, G, check_plan, planted_input
from site_rules_common import is_n_table

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L, N_QUERY = 70, 5000, 25


def _run(argv, ok=True, env=None):
    p = subprocess.run([sys.executable, "-m", "tracs_amd", "distance"] + argv + ["--loglevel", "INFO"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=dict(os.environ, **(env or {})))
    if ok:
        assert p.returncode == 0, (argv, p.stdout[-1500:] + p.stderr[-3000:])
    return p


def _bed(path, mask):
    from tracs_amd.sites import kept_runs
    with open(path, "w") as fh:
        for s, e in kept_runs(mask, len(mask)):
            fh.write("alignment\t%d\t%d\n" % (s, e))
    return path


def _write_set(td, tag, seqs, names, n_query):
    """<tag>/aln_combined.fasta (every record), query_combined.fasta + db.fasta (the records split at n_query) -> their paths"""
    from tracs_amd import synth
    d = td / tag
    d.mkdir()
    out = {"aln": str(d / "aln_combined.fasta"), "query": str(d / "query_combined.fasta"), "db": str(d / "db.fasta")}
    synth.write_fasta(out["aln"], seqs, names=names, width=80)
    synth.write_fasta(out["query"], seqs[:n_query], names=names[:n_query])
    synth.write_fasta(out["db"], seqs[n_query:], names=names[n_query:], width=61)
    return out


def _make(td, hiplib, n, length, with_files):
    """the planted input, its expectation, the full files and the files with the dropped records (and columns) deleted"""
    from tracs_amd import synth
    isn = is_n_table(hiplib)
    seqs, keep, plan = planted_input(n, length, isn, n_query=N_QUERY, with_files=with_files)
    e = check_plan(seqs, isn, keep, plan, N_QUERY)
    names = ["s%d" % i for i in range(n)]
    rows = e["kept_samples"]
    cols = e["kept_sites"] if with_files else np.ones(length, bool)          # (the sample rule alone: no column goes)
    f = {"e": e, "seqs": seqs, "keep": keep, "names": names, "td": str(td), "n": n, "L": length}
    f["full"] = _write_set(td, "full", seqs, names, N_QUERY)
    f["cut"] = _write_set(td, "cut", seqs[rows][:, cols], [nm for nm, k in zip(names, rows) if k], int(rows[:N_QUERY].sum()))
    f["rule"] = ["--max-sample-n-share", repr(G)]
    if with_files:
        f["rule"] += ["--mask", _bed(str(td / "mask.bed"), ~keep), "--max-n-share", repr(F)]
    iso, _ = synth.dates(n, seed=4)
    f["meta"], f["meta_kept_only"] = str(td / "dates.csv"), str(td / "dates_kept.csv")
    with open(f["meta"], "w") as fa, open(f["meta_kept_only"], "w") as fb:
        fa.write("sample,date\n")
        fb.write("sample,date\n")
        for nm, day, k in zip(names, iso, rows):
            fa.write("%s,%s\n" % (nm, day))
            if k:
                fb.write("%s,%s\n" % (nm, day))
    f["groups"] = str(td / "groups.csv")
    with open(f["groups"], "w") as fh:
        fh.write("sample,group\n")
        for i, nm in enumerate(names):
            fh.write("%s,%s\n" % (nm, "" if i % 7 == 0 else "g%d" % (i % 3)))
    return f


@pytest.fixture(scope="module")
def both(tmp_path_factory, hiplib):
    """70 x 5000 with file rules + --max-n-share + the sample rule"""
    return _make(tmp_path_factory.mktemp("sample_rules_both"), hiplib, N, L, True)


@pytest.fixture(scope="module")
def alone(tmp_path_factory, hiplib):
    """70 x 5000 with the sample rule alone"""
    return _make(tmp_path_factory.mktemp("sample_rules_alone"), hiplib, N, L, False)


VARIANTS = {
    "plain": ([], {}),
    "meta": (["--meta", "META"], {}),
    "meta K": (["--meta", "META", "-K", "KMED"], {}),                   # KMED: see _median_k
    "filter": (["--filter"], {}),
    "msa-db": (["--msa-db", "DB"], {}),
    "nearest": (["--nearest", "3"], {}),
    "mst": (["--mst", "snp"], {}),
    "histogram groups": (["--histogram", "--groups", "GROUPS"], {}),
    "arrays meta": (["--meta", "META"], {"TRACS_DISTANCE_ARRAYS": "1"}),
    "meta without the dropped": (["--meta", "META_KEPT"], {}),
}


def _median_k(f, tag):
    """a -K that cuts: the median `expected K` of the ordinary run with dates on the cut file, rounded up (-K takes an integer)
    -> (K as text, the number of rows of that run)"""
    out = os.path.join(f["td"], "%s_k_probe.csv" % tag)
    _run(["--msa", f["cut"]["aln"], "--meta", f["meta"], "-o", out])
    ks = sorted(float(ln.split(",")[5]) for ln in open(out).read().split("\n")[1:] if ln)
    k = max(1, math.ceil(ks[len(ks) // 2]))
    assert ks[0] <= k < ks[-1]                                                          # some pairs within it, some beyond
    return str(k), len(ks)


def _compare(f, variant, tag):
    extra, env = VARIANTS[variant]
    kmed, n_all = _median_k(f, tag) if "KMED" in extra else (None, None)

    def argv(side):
        msa = f[side]["query"] if variant == "msa-db" else f[side]["aln"]
        sub = {"META": f["meta"], "META_KEPT": f["meta_kept_only"], "DB": f[side]["db"], "GROUPS": f["groups"], "KMED": kmed}
        return ["--msa", msa] + [sub.get(x, x) for x in extra]
    out_rule, out_cut = (os.path.join(f["td"], "%s_%s_%s.csv" % (tag, variant.replace(" ", "_"), k)) for k in ("rule", "cut"))
    p = _run(argv("full") + ["-o", out_rule] + f["rule"], env=env)
    _run(argv("cut") + ["-o", out_cut], env=env)
    got, want = open(out_rule, "rb").read(), open(out_cut, "rb").read()
    assert got == want and got.count(b"\n") > 1
    if kmed is not None:
        assert got.count(b"\n") - 1 < n_all                                             # -K removed rows
    e = f["e"]
    n_read = N_QUERY + (f["n"] - N_QUERY) if variant == "msa-db" else f["n"]
    line = "kept %d of %d samples" % (int(e["kept_samples"].sum()), n_read)
    assert p.stderr.count("Sample rule for") == 1 and line in p.stderr, p.stderr[-2000:]
    return p, got


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rules_equal_the_run_on_the_cut_files(both, variant):
    p, got = _compare(both, variant, "both")
    e, keep = both["e"], both["keep"]
    line = "kept %d of %d columns (%d dropped by --mask / --keep, %d by --max-n-share)" % (e["kept_sites"].sum(), L, (~keep).sum(),
                                                                                           keep.sum() - e["kept_sites"].sum())
    assert p.stderr.count("Site rules for") == 1 and line in p.stderr, p.stderr[-2000:]
    if variant == "plain":                      # the rules changed something: neither the plain run nor the site rules alone give this
        td = both["td"]
        plain, sites_only = os.path.join(td, "plain.csv"), os.path.join(td, "sites_only.csv")
        _run(["--msa", both["full"]["aln"], "-o", plain])
        _run(["--msa", both["full"]["aln"], "-o", sites_only] + both["rule"][2:])
        assert open(plain, "rb").read() != got and open(sites_only, "rb").read() != got


@pytest.mark.parametrize("variant", ["plain", "msa-db", "nearest", "histogram groups"])
def test_sample_rule_alone_equals_the_run_without_the_records(alone, variant):
    p, got = _compare(alone, variant, "alone")
    assert "Site rules for" not in p.stderr


@pytest.mark.parametrize("with_files", [False, True], ids=["sample rule alone", "with site rules"])
def test_larger_alignment(tmp_path_factory, hiplib, with_files):
    """131 x 30001: more than 64 samples on either side of the selection, a last group that is not full"""
    f = _make(tmp_path_factory.mktemp("sample_rules_131"), hiplib, 131, 30001, with_files)
    _compare(f, "plain", "big")


def test_samples_out(both):
    td = both["td"]
    out, csv, again = os.path.join(td, "so.csv"), os.path.join(td, "samples.csv"), os.path.join(td, "so_report.csv")
    _run(["--msa", both["full"]["aln"], "-o", out, "--samples-out", csv] + both["rule"])
    e = both["e"]
    want = "sample,MSA file,N sites,sites,kept\n" + "".join(
        "%s,aln,%d,%d,%d\n" % (nm, c, e["rule_sites"], k) for nm, c, k in zip(both["names"], e["n_counts"], e["kept_samples"]))
    assert open(csv).read() == want
    # G = 1 is the report-only run: the same counts, everything kept, the distances of the site rules alone
    _run(["--msa", both["full"]["aln"], "-o", again, "--samples-out", csv, "--max-sample-n-share", "1"] + both["rule"][2:])
    rows = [ln.rstrip("\n").split(",") for ln in open(csv)][1:]
    assert [int(r[2]) for r in rows] == e["n_counts"].tolist() and all(r[4] == "1" for r in rows)
    sites_only = os.path.join(td, "sites_only2.csv")
    _run(["--msa", both["full"]["aln"], "-o", sites_only] + both["rule"][2:])
    assert open(again, "rb").read() == open(sites_only, "rb").read()


def test_a_file_emptied_by_the_rule_is_refused(both):
    td = both["td"]
    out = os.path.join(td, "refused.csv")
    p = _run(["--msa", both["full"]["aln"], "-o", out, "--max-sample-n-share", "0"], ok=False)          # every record has an N somewhere
    assert p.returncode != 0 and "no sample left after the sample rule" in p.stderr
    # two files: the database is left with nothing although the query keeps records
    from tracs_amd import synth
    q, db = os.path.join(td, "clean_query_combined.fasta"), os.path.join(td, "dirty_db.fasta")
    clean = np.full((3, 40), ord("A"), np.uint8)
    clean[1, 5] = ord("C")
    dirty = clean.copy()
    dirty[:, 7] = ord("N")
    synth.write_fasta(q, clean, names=["q0", "q1", "q2"])
    synth.write_fasta(db, dirty, names=["d0", "d1", "d2"])
    p = _run(["--msa", q, "--msa-db", db, "-o", out, "--max-sample-n-share", "0"], ok=False)
    assert p.returncode != 0 and "no sample left after the sample rule" in p.stderr
    # one surviving record in a one-file run is allowed: no pair, the header alone
    one = os.path.join(td, "one_combined.fasta")
    mixed = dirty.copy()
    mixed[1, 7] = ord("A")
    synth.write_fasta(one, mixed, names=["a", "b", "c"])
    _run(["--msa", one, "-o", out, "--max-sample-n-share", "0"])
    assert open(out).read().count("\n") == 1


def test_api_info_and_the_order_of_the_rules(both, oracle):
    """through api.pairsnp_arrays: names, rows and cols are the surviving samples, info holds what the rule saw, the distances are the
    oracle's on seqs[rows][:, cols] -- with the N share counted over the survivors"""
    from tracs_amd import api
    from tracs_amd.sites import Sites
    e, seqs, keep = both["e"], both["seqs"], both["keep"]
    info = {}
    r, c, d, names, filt, nn = api.pairsnp_arrays([both["full"]["aln"]], sites=Sites(keep), max_sample_n_share=G, max_n_share=F, info=info)
    er, ec, ed, enn = oracle.pairsnp_arrays(seqs[e["kept_samples"]][:, e["kept_sites"]])
    assert np.array_equal(r, er) and np.array_equal(c, ec) and np.array_equal(d, ed) and np.array_equal(nn, enn)
    assert names == [nm for nm, k in zip(both["names"], e["kept_samples"]) if k]
    assert info["source_names"] == both["names"] and np.array_equal(info["n_counts"], e["n_counts"])
    assert np.array_equal(info["kept"], e["kept_samples"]) and info["rule_sites"] == e["rule_sites"] and info["seqlen"] == e["kept_sites"].sum()
    with pytest.raises(ValueError):
        api.pairsnp_arrays([both["full"]["aln"]], sites=Sites(keep, 3), max_sample_n_share=G)
    names_h, hist = api.distance_histogram([both["full"]["aln"]], sites=Sites(keep), max_sample_n_share=G, max_n_share=F)
    assert names_h == names
    v, cnt = np.unique(ed, return_counts=True)
    assert np.array_equal(hist["snp"]["value"], v) and np.array_equal(hist["snp"]["ungrouped"], cnt)


# ---- the pair rule ---------------------------------------------------------------------------------------------------------------

def _rows(path):
    """the data rows of a distance CSV: [(line, sampleA, sampleB, SNP distance, sites considered)]"""
    out = []
    for ln in open(path).read().split("\n")[1:]:
        if ln:
            f = ln.split(",")
            out.append((ln, f[0], f[1], int(f[3]), int(f[7])))
    return out


@pytest.fixture(scope="module")
def unruled(alone):
    """the ordinary run on the full file, and M: a value of `sites considered` that occurs, near the median"""
    out = os.path.join(alone["td"], "unruled.csv")
    _run(["--msa", alone["full"]["aln"], "-o", out])
    rows = _rows(out)
    nn = sorted(r[4] for r in rows)
    m = nn[len(nn) // 2]
    kept = [r for r in rows if r[4] >= m]
    assert 0 < len(kept) < len(rows) and any(r[4] == m for r in rows)                 # removes a pair, keeps a pair, hits the boundary
    return {"path": out, "rows": rows, "kept": kept, "M": m, "header": open(out).readline()}


def test_min_sites_full_output(alone, unruled):
    out = os.path.join(alone["td"], "min_sites.csv")
    _run(["--msa", alone["full"]["aln"], "-o", out, "--min-sites", str(unruled["M"])])
    assert open(out).read() == unruled["header"] + "".join(r[0] + "\n" for r in unruled["kept"])
    # with -D on top: the same filter over the rows within the threshold
    d_cut = sorted(r[3] for r in unruled["kept"])[len(unruled["kept"]) // 2]
    _run(["--msa", alone["full"]["aln"], "-o", out, "--min-sites", str(unruled["M"]), "-D", str(d_cut)])
    want = [r for r in unruled["kept"] if r[3] <= d_cut]
    assert 0 < len(want) < len(unruled["kept"])
    assert open(out).read() == unruled["header"] + "".join(r[0] + "\n" for r in want)
    # and through the array route
    _run(["--msa", alone["full"]["aln"], "-o", out, "--min-sites", str(unruled["M"])], env={"TRACS_DISTANCE_ARRAYS": "1"})
    assert open(out).read() == unruled["header"] + "".join(r[0] + "\n" for r in unruled["kept"])


def test_min_sites_nearest(alone, unruled):
    k = 3
    out = os.path.join(alone["td"], "min_sites_nearest.csv")
    _run(["--msa", alone["full"]["aln"], "-o", out, "--min-sites", str(unruled["M"]), "--nearest", str(k)])
    index = {nm: i for i, nm in enumerate(alone["names"])}
    cand = {}
    for ln, a, b, d, nn in unruled["kept"]:
        cand.setdefault(index[a], []).append((d, index[b], nn))
        cand.setdefault(index[b], []).append((d, index[a], nn))
    want = []
    for s in sorted(cand):
        for d, j, nn in sorted(cand[s])[:k]:                                          # SNP distance, then input order
            want.append((alone["names"][s], alone["names"][j], d, nn))
    got = [(r[1], r[2], r[3], r[4]) for r in _rows(out)]
    assert got == want
    plain = os.path.join(alone["td"], "plain_nearest.csv")
    _run(["--msa", alone["full"]["aln"], "-o", plain, "--nearest", str(k)])
    assert [(r[1], r[2], r[3], r[4]) for r in _rows(plain)] != got                    # the rule changed the selection


def test_min_sites_forest(alone, unruled):
    out = os.path.join(alone["td"], "min_sites_mst.csv")
    _run(["--msa", alone["full"]["aln"], "-o", out, "--min-sites", str(unruled["M"]), "--mst", "snp"])
    forest = _rows(out)
    lines = {r[0] for r in unruled["kept"]}
    assert 0 < len(forest) < alone["n"] and all(r[0] in lines for r in forest)        # every row is a row of the filtered full output
    index = {nm: i for i, nm in enumerate(alone["names"])}

    def graph(rows):
        return [index[r[1]] for r in rows], [index[r[2]] for r in rows], [r[3] for r in rows]
    ds = sorted({r[3] for r in unruled["kept"]})
    for t in (ds[0], ds[len(ds) // 4], ds[len(ds) // 2], ds[-1]):
        assert fr.threshold_partition(alone["n"], *graph(forest), t) == fr.threshold_partition(alone["n"], *graph(unruled["kept"]), t), t
    # the forest of the eligible pairs is not the forest of all pairs with the ineligible rows struck out
    i, j, w = graph(unruled["kept"])
    ref = fr.forest(alone["n"], i, j, np.asarray(w, np.uint32))
    assert sorted((index[r[1]], index[r[2]]) for r in forest) == sorted((i[e], j[e]) for e in ref.tolist())


def test_min_sites_histogram(alone, unruled):
    out = os.path.join(alone["td"], "min_sites_hist.csv")
    _run(["--msa", alone["full"]["aln"], "-o", out, "--min-sites", str(unruled["M"]), "--histogram"])
    v, cnt = np.unique([r[3] for r in unruled["kept"]], return_counts=True)
    want = "column,distance,within,between,ungrouped,MSA file\n" + "".join("snp,%d,0,0,%d,aln\n" % (a, b) for a, b in zip(v, cnt))
    assert open(out).read() == want


def test_both_rules_together(both):
    """--min-sites counts the sites that the site rules kept, over the pairs of the surviving samples"""
    td = both["td"]
    cut, ruled = os.path.join(td, "cut_plain.csv"), os.path.join(td, "all_rules.csv")
    _run(["--msa", both["cut"]["aln"], "-o", cut])
    rows = _rows(cut)
    nn = sorted(r[4] for r in rows)
    m = nn[len(nn) // 3]
    kept = [r for r in rows if r[4] >= m]
    assert 0 < len(kept) < len(rows)
    _run(["--msa", both["full"]["aln"], "-o", ruled, "--min-sites", str(m)] + both["rule"])
    assert open(ruled).read() == open(cut).readline() + "".join(r[0] + "\n" for r in kept)
