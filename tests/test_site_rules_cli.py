"""`tracs distance` under site rules, through the command line: a run with --mask / --keep / --max-n-share on an alignment writes,
byte for byte, what the run without any site option writes on the alignment with the kept columns only."""
import os
import subprocess
import sys

import numpy as np
import pytest

from site_rules_common import is_n_table, standard_files_keep, standard_input, standard_rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L, N_QUERY = 70, 5000, 25


def _run(argv, ok=True):
    p = subprocess.run([sys.executable, "-m", "tracs_amd", "distance"] + argv + ["--loglevel", "INFO"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    if ok:
        assert p.returncode == 0, (argv, p.stdout[-1500:] + p.stderr[-3000:])
    return p


def _bed(path, keep_or_mask, contig="alignment"):
    """BED of the True runs of a bool array"""
    from tracs_amd.sites import kept_runs
    with open(path, "w") as fh:
        fh.write("# columns\n")
        for s, e in kept_runs(keep_or_mask, len(keep_or_mask)):
            fh.write("%s\t%d\t%d\n" % (contig, s, e))
    return path


@pytest.fixture(scope="module")
def files(tmp_path_factory, hiplib):
    from tracs_amd import synth
    td = tmp_path_factory.mktemp("site_rules_cli")
    isn = is_n_table(hiplib)
    seqs, _ = standard_input(N, L)
    keep, max_n, kept = standard_rule(seqs, isn)
    assert not np.array_equal(keep, kept) and kept.sum() % 128 != 0
    names = ["s%d" % i for i in range(N)]
    f = {"kept": kept, "keep": keep, "seqs": seqs, "td": str(td)}
    for side, cols in (("full", np.ones(L, bool)), ("cut", kept)):
        d = td / side
        d.mkdir()
        f[side] = str(d / "aln_combined.fasta")
        f[side + "_query"] = str(d / "query_combined.fasta")
        f[side + "_db"] = str(d / "db.fasta")
        synth.write_fasta(f[side], seqs[:, cols], names=names, width=80)
        synth.write_fasta(f[side + "_query"], seqs[:N_QUERY][:, cols], names=names[:N_QUERY])
        synth.write_fasta(f[side + "_db"], seqs[N_QUERY:][:, cols], names=names[N_QUERY:], width=61)
    f["mask"] = _bed(str(td / "mask.bed"), ~keep)
    iso, _ = synth.dates(N, seed=4)
    f["meta"] = str(td / "dates.csv")
    with open(f["meta"], "w") as fh:
        fh.write("sample,date\n")
        for nm, day in zip(names, iso):
            fh.write("%s,%s\n" % (nm, day))
    f["groups"] = str(td / "groups.csv")
    with open(f["groups"], "w") as fh:
        fh.write("sample,group\n")
        for i, nm in enumerate(names):
            fh.write("%s,%s\n" % (nm, "" if i % 7 == 0 else "g%d" % (i % 3)))
    return f


VARIANTS = {
    "plain": [],
    "meta": ["--meta", "META"],
    "filter meta": ["--filter", "--meta", "META"],
    "D": ["-D", "40"],
    "msa-db": ["--msa-db", "DB"],
    "nearest": ["--nearest", "3"],
    "mst": ["--mst", "snp"],
    "histogram groups": ["--histogram", "--groups", "GROUPS"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rule_equals_the_run_on_the_cut_alignment(files, variant):
    def argv(side):
        msa = files[side + "_query"] if variant == "msa-db" else files[side]
        sub = {"META": files["meta"], "DB": files[side + "_db"], "GROUPS": files["groups"]}
        return ["--msa", msa] + [sub.get(x, x) for x in VARIANTS[variant]]
    out_rule, out_cut, out_full = (os.path.join(files["td"], "%s_%s.csv" % (variant.replace(" ", "_"), k)) for k in ("rule", "cut", "full"))
    p = _run(argv("full") + ["-o", out_rule, "--mask", files["mask"], "--max-n-share", "0.2"])
    _run(argv("cut") + ["-o", out_cut])
    got, want = open(out_rule, "rb").read(), open(out_cut, "rb").read()
    assert got == want and got.count(b"\n") > 1
    # one INFO line: kept K of L, dropped by the files, dropped by the N rule (over both files with --msa-db)
    kept, keep = files["kept"], files["keep"]
    line = "kept %d of %d columns (%d dropped by --mask / --keep, %d by --max-n-share)" % (kept.sum(), L, (~keep).sum(), keep.sum() - kept.sum())
    assert p.stderr.count("Site rules for") == 1 and line in p.stderr, p.stderr[-2000:]
    if variant == "plain":                      # ... and the rule changed something: not the output of the run without it
        _run(argv("full") + ["-o", out_full])
        assert open(out_full, "rb").read() != got


def test_sites_out_feeds_keep(files):
    td = files["td"]
    first, again, bed = (os.path.join(td, x) for x in ("so_first.csv", "so_again.csv", "kept.bed"))
    _run(["--msa", files["full"], "-o", first, "--mask", files["mask"], "--max-n-share", "0.2", "--sites-out", bed])
    from tracs_amd.sites import keep_bool, read_bed
    assert np.array_equal(keep_bool(L, keep=read_bed(bed)), files["kept"])
    _run(["--msa", files["full"], "-o", again, "--keep", bed])
    assert open(first, "rb").read() == open(again, "rb").read()
    # --keep with --mask: keep minus mask
    wide, minus = os.path.join(td, "wide.bed"), os.path.join(td, "minus.bed")
    k = files["kept"].copy(); k[100:357] = True       # (columns the rule drops: the mask has to take them out again)
    _bed(wide, k)
    _bed(minus, k & ~files["kept"])
    third = os.path.join(td, "so_third.csv")
    _run(["--msa", files["full"], "-o", third, "--keep", wide, "--mask", minus])
    assert open(first, "rb").read() == open(third, "rb").read()


def test_mask_reference(files):
    """a BED in contig coordinates selects the same columns as its alignment-column twin; --sites-out then speaks contig coordinates"""
    td = files["td"]
    ref = os.path.join(td, "ref.fa")
    lens = [("chrA", 1300), ("plasmid", 700), ("chrB", L - 2000)]
    with open(ref, "w") as fh:
        for name, ln in lens:
            fh.write(">%s some description\n" % name)
            for o in range(0, ln, 70):
                fh.write("A" * min(70, ln - o) + "\n")
    drop = ~standard_files_keep(L)
    drop[1250:1350] = True                      # across the first contig boundary
    drop[1999:2003] = True                      # and the second
    flat, contig = os.path.join(td, "flat.bed"), os.path.join(td, "contig.bed")
    _bed(flat, drop)
    from tracs_amd.sites import kept_runs
    with open(contig, "w") as fh:
        off = 0
        for name, ln in lens:
            local = drop[off:off + ln]
            for s, e in kept_runs(local, ln):
                fh.write("%s %d %d\n" % (name, s, e))
            off += ln
    a, b, bed = (os.path.join(td, x) for x in ("mr_flat.csv", "mr_contig.csv", "mr_kept.bed"))
    _run(["--msa", files["full"], "-o", a, "--mask", flat])
    _run(["--msa", files["full"], "-o", b, "--mask", contig, "--mask-reference", ref, "--sites-out", bed])
    assert open(a, "rb").read() == open(b, "rb").read()
    from tracs_amd.align_post import read_contigs
    from tracs_amd.sites import keep_bool, read_bed
    assert {ln.split("\t")[0] for ln in open(bed)} == {"chrA", "plasmid", "chrB"}
    assert np.array_equal(keep_bool(L, keep=read_bed(bed, read_contigs(ref))), ~drop)


def test_bed_past_the_end_is_refused(files):
    td = files["td"]
    bad, out = os.path.join(td, "bad.bed"), os.path.join(td, "bad.csv")
    with open(bad, "w") as fh:
        fh.write("alignment\t4990\t%d\n" % (L + 1))
    p = _run(["--msa", files["full"], "-o", out, "--mask", bad], ok=False)
    assert p.returncode != 0
    assert "reaches past the alignment's length (%d)" % L in p.stderr and files["full"] in p.stderr
    # and a rule that leaves nothing is refused with the library's message
    none = os.path.join(td, "none.bed")
    with open(none, "w") as fh:
        fh.write("alignment\t0\t%d\n" % L)
    p = _run(["--msa", files["full"], "-o", out, "--mask", none], ok=False)
    assert p.returncode != 0 and "no site left after the site rules" in p.stderr
