"""--msa-out / --msa-out-sites / --site-table through the command line.  The sentence every rule rests on -- a run with
a rule is the run on the alignment with the dropped columns and records deleted -- is executed: the run writes that alignment, and
the run on the written file without any rule gives the same CSV byte for byte."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from sample_rules_common import G, expected, files_keep, planted_input
from site_rules_common import is_n_table

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L, F = 70, 5000, 0.2
LUT = np.frombuffer(b"XACMGRSVTWYHKDBN", np.uint8)
CONTIGS = [("chrA", 1800), ("chrB", L - 1800)]


def _run(argv, env=None):
    p = subprocess.run([sys.executable, "-m", "tracs_amd", "distance"] + argv + ["--loglevel", "INFO"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, (argv, p.stdout[-1500:] + p.stderr[-3000:])
    return p


def _read_fasta(path):
    op = gzip.open if path.endswith(".gz") else open
    names, rows = [], []
    with op(path, "rb") as fh:
        lines = fh.read().split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1                      # ">name\nSEQ\n" per record, one line per sequence
    for k in range(0, len(lines) - 1, 2):
        assert lines[k].startswith(b">")
        names.append(lines[k][1:].decode())
        rows.append(np.frombuffer(lines[k + 1], np.uint8))
    return names, np.stack(rows)


def _census_numpy(masks):
    counts = np.stack([(masks == m).sum(axis=0) for m in (1, 2, 4, 8, 15)] + [np.isin(masks, (3, 5, 6, 7, 9, 10, 11, 12, 13, 14)).sum(axis=0)])
    differs = np.zeros(masks.shape[1], bool)
    for a in range(1, 15):
        for b in range(a + 1, 15):
            if a & b == 0:
                differs |= (masks == a).any(axis=0) & (masks == b).any(axis=0)
    return counts, differs


def _bed(path, drop, contigs=None):
    from tracs_amd.sites import kept_runs
    with open(path, "w") as fh:
        if contigs is None:
            for s, e in kept_runs(drop, len(drop)):
                fh.write("alignment\t%d\t%d\n" % (s, e))
        else:
            off = 0
            for name, ln in contigs:
                for s, e in kept_runs(drop[off:off + ln], ln):
                    fh.write("%s\t%d\t%d\n" % (name, s, e))
                off += ln
    return path


@pytest.fixture(scope="module")
def files(tmp_path_factory, hiplib):
    """the input, its rules, and ONE run with every new option: the CSV, the compared alignment (.gz), the site table"""
    from tracs_amd import synth
    td = tmp_path_factory.mktemp("msa_out_cli")
    isn = is_n_table(hiplib)
    table = np.array([hiplib.tracs_debug_iupac_mask(ch) for ch in range(256)], np.uint8)
    seqs, keep, _ = planted_input(N, L, isn)
    rng = np.random.default_rng(3)
    lower = (rng.random(seqs.shape) < 0.03) & (seqs >= 65) & (seqs <= 90)       # lower case, '-' and bytes that are no letter:
    seqs[lower] += 32                                                           # the output is canonical, not a copy
    seqs[rng.random(seqs.shape) < 0.002] = ord("-")
    seqs[2, 777], seqs[3, 778] = ord("?"), ord("*")
    e = expected(seqs, isn, keep, G, F)
    ks, kc = e["kept_samples"], e["kept_sites"]
    assert 1 <= (~ks).sum() < N and kc.sum() < keep.sum() < L                   # a sample goes, the mask and the N share drop columns
    names = ["s%d" % i for i in range(N)]
    f = dict(td=str(td), seqs=seqs, ks=ks, kc=kc, names=names, table=table, text=LUT[table[seqs[ks][:, kc]]])
    assert (f["text"] != seqs[ks][:, kc]).any()
    for d in ("in", "out", "diff", "plain"):
        (td / d).mkdir()
    f["msa"] = str(td / "in" / "aln_combined.fasta")
    synth.write_fasta(f["msa"], seqs, names=names, width=80)
    f["mask"] = _bed(str(td / "mask.bed"), ~keep)
    iso, _ = synth.dates(N, seed=4)
    f["meta"] = str(td / "dates.csv")
    with open(f["meta"], "w") as fh:
        fh.write("sample,date\n")
        for nm, day in zip(names, iso):
            fh.write("%s,%s\n" % (nm, day))
    f["rules"] = ["--msa", f["msa"], "--mask", f["mask"], "--max-n-share", str(F), "--max-sample-n-share", str(G)]
    f["out"], f["table_csv"], f["csv"] = str(td / "out" / "aln_combined.fasta.gz"), str(td / "table.csv"), str(td / "with.csv")
    f["log"] = _run(f["rules"] + ["-o", f["csv"], "--msa-out", f["out"], "--site-table", f["table_csv"]]).stderr
    return f


def test_the_file_is_the_compared_alignment(files):
    names, rows = _read_fasta(files["out"])
    assert names == [nm for nm, k in zip(files["names"], files["ks"]) if k]
    assert rows.shape == files["text"].shape and np.array_equal(rows, files["text"])
    # one gzip member per record
    import zlib
    data, members = open(files["out"], "rb").read(), 0
    while data:
        d = zlib.decompressobj(16 + zlib.MAX_WBITS)
        d.decompress(data)
        data, members = d.unused_data, members + 1
    assert members == len(names)
    _, differs = _census_numpy(files["table"][files["seqs"][files["ks"]][:, files["kc"]]])
    assert "(%d records, %d columns, %d differing)" % (len(names), rows.shape[1], differs.sum()) in files["log"], files["log"][-1500:]
    assert files["log"].count("Compared alignment of") == 1 and files["log"].count("Site table for") == 1


@pytest.mark.parametrize("variant", ["plain", "meta", "filter meta"])
def test_the_definition_executed(files, variant):
    """the run with the rules == the run without any rule on the alignment the first one wrote"""
    extra = {"plain": [], "meta": ["--meta", files["meta"]], "filter meta": ["--filter", "--meta", files["meta"]]}[variant]
    a, b = (os.path.join(files["td"], "def_%s_%s.csv" % (variant.replace(" ", "_"), k)) for k in ("rule", "file"))
    _run(files["rules"] + extra + ["-o", a])
    _run(["--msa", files["out"]] + extra + ["-o", b])
    got, want = open(a, "rb").read(), open(b, "rb").read()
    assert got == want and got.count(b"\n") > 100
    if variant == "plain":
        assert got == open(files["csv"], "rb").read()                    # ... and the run that wrote the files wrote this CSV too


def _csv_columns(path):
    rows = [ln.rstrip("\n").split(",") for ln in open(path)][1:]
    return [(r[0], r[1], r[3]) for r in rows], [int(r[7]) for r in rows]


def test_differing_columns(files, oracle):
    td = files["td"]
    out, tab, csv = os.path.join(td, "diff", "aln_combined.fasta"), os.path.join(td, "diff_table.csv"), os.path.join(td, "diff_run.csv")
    p = _run(files["rules"] + ["-o", csv, "--msa-out", out, "--msa-out-sites", "differing", "--site-table", tab])
    assert open(csv, "rb").read() == open(files["csv"], "rb").read()      # what is written does not change what is computed
    masks = files["table"][files["seqs"][files["ks"]][:, files["kc"]]]
    _, differs = _census_numpy(masks)
    names, rows = _read_fasta(out)
    assert 0 < differs.sum() < masks.shape[1]
    assert rows.shape == (int(files["ks"].sum()), int(differs.sum())) and np.array_equal(rows, files["text"][:, differs])
    table_differs = [int(ln.rstrip("\n").split(",")[8]) for ln in list(open(tab))[1:]]
    assert len(table_differs) == masks.shape[1] and sum(table_differs) == rows.shape[1]
    assert "(%d records, %d columns, %d differing)" % (len(names), rows.shape[1], rows.shape[1]) in p.stderr
    # a run on it: the same pairs and SNP distances as the run on the kept alignment, `sites considered` over those columns only
    again = os.path.join(td, "diff_again.csv")
    _run(["--msa", out, "-o", again])
    pairs_d, sites_d = _csv_columns(again)
    pairs_k, sites_k = _csv_columns(files["csv"])
    assert pairs_d == pairs_k and len(pairs_d) > 100
    r, c, d, nn = oracle.pairsnp_arrays(rows)
    assert sites_d == [int(x) for x in nn] and sites_d != sites_k
    assert [int(x) for x in d] == [int(p3) for _, _, p3 in pairs_d]


NO_EFFECT = {
    "nearest": (["--nearest", "3"], None),
    "mst": (["--mst", "snp"], None),
    "histogram": (["--histogram"], None),
    "arrays": ([], {"TRACS_DISTANCE_ARRAYS": "1"}),
}


@pytest.mark.parametrize("variant", list(NO_EFFECT))
def test_no_effect_on_the_run(files, variant):
    """on every route: the CSV with the new options is the CSV without them, and the files are the ones the plain run wrote"""
    extra, env = NO_EFFECT[variant]
    td = files["td"]
    a, b = (os.path.join(td, "ne_%s_%s.csv" % (variant, k)) for k in ("with", "without"))
    out, tab = os.path.join(td, "plain", "ne_%s.fasta" % variant), os.path.join(td, "ne_%s_table.csv" % variant)
    p = _run(files["rules"] + extra + ["-o", a, "--msa-out", out, "--site-table", tab], env=env)
    _run(files["rules"] + extra + ["-o", b], env=env)
    got = open(a, "rb").read()
    assert got == open(b, "rb").read() and got.count(b"\n") > 1
    assert open(out, "rb").read() == gzip.open(files["out"], "rb").read()         # plain text here, .gz there: the same records
    assert open(tab, "rb").read() == open(files["table_csv"], "rb").read()
    assert p.stderr.count("Compared alignment of") == 1 and p.stderr.count("Site table for") == 1
    assert p.stderr.count("Site rules for") == 1 and p.stderr.count("Sample rule for") == 1


def test_site_table(files):
    masks = files["table"][files["seqs"][files["ks"]][:, files["kc"]]]
    counts, differs = _census_numpy(masks)
    lines = open(files["table_csv"]).read().split("\n")
    assert lines[0] == "contig,position,A,C,G,T,N,other,differs" and lines[-1] == ""
    rows = [ln.split(",") for ln in lines[1:-1]]
    pos = np.flatnonzero(files["kc"])
    assert len(rows) == len(pos)
    assert [r[0] for r in rows] == ["alignment"] * len(pos) and [int(r[1]) for r in rows] == pos.tolist()
    got = np.array([[int(x) for x in r[2:8]] for r in rows]).T
    assert np.array_equal(got, counts) and (got.sum(axis=0) == files["ks"].sum()).all()
    assert [int(r[8]) for r in rows] == differs.astype(int).tolist()


def test_site_table_in_contig_coordinates(files):
    td = files["td"]
    ref, mask, tab, csv = (os.path.join(td, x) for x in ("ref.fa", "contig_mask.bed", "contig_table.csv", "contig.csv"))
    with open(ref, "w") as fh:
        for name, ln in CONTIGS:
            fh.write(">%s description\n" % name)
            for o in range(0, ln, 70):
                fh.write("A" * min(70, ln - o) + "\n")
    _bed(mask, ~files_keep(L), CONTIGS)
    _run(["--msa", files["msa"], "--mask", mask, "--mask-reference", ref, "--max-n-share", str(F), "--max-sample-n-share", str(G),
          "-o", csv, "--site-table", tab])
    assert open(csv, "rb").read() == open(files["csv"], "rb").read()
    flat = [ln.split(",") for ln in open(files["table_csv"]).read().split("\n")[1:-1]]
    rows = [ln.split(",") for ln in open(tab).read().split("\n")[1:-1]]
    pos = np.flatnonzero(files["kc"])
    cut = CONTIGS[0][1]
    first_b = int(np.searchsorted(pos, cut))
    assert 0 < first_b < len(pos) and len(rows) == len(pos)
    assert [r[0] for r in rows] == ["chrA"] * first_b + ["chrB"] * (len(pos) - first_b)          # the contig changes at the right row
    assert [int(r[1]) for r in rows] == [int(x) if x < cut else int(x) - cut for x in pos]
    assert [r[2:] for r in rows] == [r[2:] for r in flat]


def test_gzip_output_reads_back(files):
    """Alignment.from_fasta on the .gz the run wrote == packing the expected text: the same names, the same bytes"""
    import torch
    from tracs_amd import device as dev
    from tracs_amd.multigpu import _DeviceBytes

    def plane_bytes(aln):
        torch.cuda.synchronize()
        return torch.as_tensor(_DeviceBytes(aln.planes_ptr(), aln.nbytes), device="cuda").cpu().numpy().copy()
    got = dev.Alignment.from_fasta([files["out"]])
    assert got.names == [nm for nm, k in zip(files["names"], files["ks"]) if k]
    assert (got.n, got.L) == files["text"].shape
    twin = dev.Alignment(*files["text"].shape)
    twin.pack(np.ascontiguousarray(files["text"]))
    assert np.array_equal(plane_bytes(got), plane_bytes(twin))
    assert np.array_equal(got.unpack().cpu().numpy(), files["text"])
    got.close()
    twin.close()


def test_without_any_rule_the_input_is_canonicalised(files):
    td = files["td"]
    out, csv, plain = os.path.join(td, "plain", "aln_combined.fasta"), os.path.join(td, "norule.csv"), os.path.join(td, "norule_plain.csv")
    p = _run(["--msa", files["msa"], "-o", csv, "--msa-out", out])
    _run(["--msa", files["msa"], "-o", plain])
    assert open(csv, "rb").read() == open(plain, "rb").read()
    names, rows = _read_fasta(out)
    assert names == files["names"] and np.array_equal(rows, LUT[files["table"][files["seqs"]]])
    assert "Site rules for" not in p.stderr and p.stderr.count("Compared alignment of") == 1
