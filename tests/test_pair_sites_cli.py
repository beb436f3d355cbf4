"""`tracs pair-sites` through the command line: for the pairs of a `distance` file the rows number the SNP distance
and the rows with dropped = 0 the filtered SNP distance, under site and sample rules too; contig and position point into the input
FASTA at the letters written.  The parser and error cases at the end need no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = "XACMGRSVTWYHKDBN"
N, L = 24, 6000
CONTIGS = [("chrA", 2500), ("chrB", L - 2500)]
_CACHE = {}


def _cli(monkeypatch, argv):
    """`tracs <argv>` in this process (one GPU context for the whole module)"""
    from tracs_amd import __main__ as M
    monkeypatch.setattr(sys, "argv", ["tracs"] + [str(x) for x in argv])
    M.main()


def _mask_table():
    t = np.full(256, 15, np.uint8)
    for m, ch in enumerate(LETTERS):
        if 1 <= m <= 14:
            t[ord(ch)] = t[ord(ch.lower())] = m
    return t


def _seqs():
    """24 x 6000: SNPs, a dense run in every other sample (the filter drops it), N, partial codes, lower case; columns 3000 .. 3059
    are N in most samples (--max-n-share drops them) and sample 7 is N over a third of its length (--max-sample-n-share drops it)"""
    if "seqs" not in _CACHE:
        rng = np.random.default_rng(424)
        acgt = np.frombuffer(b"ACGT", np.uint8)
        base = acgt[rng.integers(0, 4, L)]
        seqs = np.tile(base, (N, 1))
        for s in range(N):
            hit = rng.random(L) < 0.004
            seqs[s, hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
            if s % 2 == 0:
                start = int(rng.integers(0, L - 300))
                hit = np.zeros(L, bool)
                hit[start:start + 300] = rng.random(300) < 0.2
                seqs[s, hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
            for chars, p in ((b"N-", 0.01), (b"MRWSYK", 0.004), (b"acgt", 0.01)):
                hit = rng.random(L) < p
                seqs[s, hit] = np.frombuffer(chars, np.uint8)[rng.integers(0, len(chars), int(hit.sum()))]
        seqs[rng.random(N) < 0.8, 3000:3060] = ord("N")
        seqs[7, 1000:3000] = ord("N")
        seqs.setflags(write=False)
        _CACHE["seqs"] = seqs
    return _CACHE["seqs"]


def _names():
    return ["iso%02d" % i for i in range(N)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from tracs_amd import synth
    td = str(tmp_path_factory.mktemp("pair_sites_cli"))
    fa = os.path.join(td, "aln.fa")
    synth.write_fasta(fa, np.array(_seqs()), names=_names(), width=70)
    ref = os.path.join(td, "ref.fa")
    with open(ref, "w") as fh:
        for name, length in CONTIGS:
            fh.write(">%s some description\n%s\n" % (name, "A" * length))
    return {"td": td, "fa": fa, "ref": ref}


def _read_rows(path):
    with open(path) as fh:
        lines = fh.read().split("\n")
    assert lines[0] == "sampleA,sampleB,contig,position,alleleA,alleleB,dropped" and lines[-1] == ""
    return [x.split(",") for x in lines[1:-1]]


def _read_distance(path):
    with open(path) as fh:
        next(fh)
        return [x.rstrip("\n").split(",") for x in fh]


def _counts(rows):
    """{(a, b): [rows, rows with dropped == 0]} and the order in which the pairs first appear"""
    out, order = {}, []
    for f in rows:
        key = (f[0], f[1])
        if key not in out:
            out[key] = [0, 0]
            order.append(key)
        out[key][0] += 1
        out[key][1] += f[6] == "0"
    return out, order


def _check_against_distance(dist_csv, sites_csv):
    pairs = _read_distance(dist_csv)
    assert len(pairs) > 5
    got, order = _counts(_read_rows(sites_csv))
    want_order = [(f[0], f[1]) for f in pairs if int(f[3]) > 0]
    assert order == want_order
    dropped_any = 0
    for f in pairs:
        rows, kept = got.get((f[0], f[1]), [0, 0])
        assert rows == int(f[3]) and kept == int(f[6]), f
        dropped_any += kept < rows
    assert dropped_any > 0


@pytest.mark.gpu
def test_rows_number_the_distances_of_a_distance_file(hiplib, files, monkeypatch):
    td, fa = files["td"], files["fa"]
    close = os.path.join(td, "close.csv")
    _cli(monkeypatch, ["distance", "--msa", fa, "--filter", "-D", "160", "-o", close])
    out = os.path.join(td, "close_sites.csv")
    # the command line itself, once, in a process of its own
    p = subprocess.run([sys.executable, "-m", "tracs_amd", "pair-sites", "--msa", fa, "--pairs", close, "--filter", "-o", out, "-t", "2"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    _check_against_distance(close, out)
    masks = _mask_table()[_seqs()]
    idx = {n: i for i, n in enumerate(_names())}
    for f in _read_rows(out)[::37]:
        assert f[2] == "alignment"
        a, b, s = masks[idx[f[0]], int(f[3])], masks[idx[f[1]], int(f[3])], int(f[3])
        assert (a & b) == 0 and f[4] == LETTERS[a] and f[5] == LETTERS[b], (f, s)
    # without --filter: the same rows, dropped = NA
    plain = os.path.join(td, "close_plain.csv")
    _cli(monkeypatch, ["pair-sites", "--msa", fa, "--pairs", close, "-o", plain])
    assert [f[:6] + ["NA"] for f in _read_rows(out)] == _read_rows(plain)


@pytest.mark.gpu
def test_rows_number_the_distances_of_a_forest_file(hiplib, files, monkeypatch):
    td, fa = files["td"], files["fa"]
    forest = os.path.join(td, "forest.csv")
    _cli(monkeypatch, ["distance", "--msa", fa, "--filter", "--mst", "snp", "-o", forest])
    assert len(_read_distance(forest)) == N - 1
    out = os.path.join(td, "forest_sites.csv")
    _cli(monkeypatch, ["pair-sites", "--msa", fa, "--pairs", forest, "--filter", "-o", out])
    _check_against_distance(forest, out)


@pytest.mark.gpu
def test_site_rules_point_into_the_input(hiplib, files, monkeypatch):
    """--mask + --mask-reference + --max-n-share: contig and position are the input's, no row lies in a dropped column, and the rows
    are those of the ruleless run on the --msa-out alignment with its positions mapped through --sites-out"""
    from tracs_amd import sites as S
    td, fa, ref = files["td"], files["fa"], files["ref"]
    bed = os.path.join(td, "mask.bed")
    with open(bed, "w") as fh:
        fh.write("chrA\t100\t400\nchrB\t0\t50\nchrB\t3000\t3500\n")
    masked = np.zeros(L, bool)
    masked[100:400] = masked[2500:2550] = masked[5500:6000] = True
    rules = ["--mask", bed, "--mask-reference", ref, "--max-n-share", "0.5"]
    dist = os.path.join(td, "ruled.csv")
    kept_bed, msa_out = os.path.join(td, "kept.bed"), os.path.join(td, "compared.fa")
    _cli(monkeypatch, ["distance", "--msa", fa, "--filter", "-D", "160", "-o", dist, "--sites-out", kept_bed, "--msa-out", msa_out] + rules)
    ruled = os.path.join(td, "ruled_sites.csv")
    _cli(monkeypatch, ["pair-sites", "--msa", fa, "--pairs", dist, "--filter", "-o", ruled] + rules)
    _check_against_distance(dist, ruled)
    rows = _read_rows(ruled)
    seqs, table = _seqs(), _mask_table()
    idx = {n: i for i, n in enumerate(_names())}
    start = {"chrA": 0, "chrB": 2500}
    kept = S.keep_bool(L, S.read_bed(kept_bed, CONTIGS), None)
    assert not kept[3000:3060].any() and not (kept & masked).any() and kept.sum() < L - masked.sum()
    for f in rows:
        col = start[f[2]] + int(f[3])
        assert 0 <= int(f[3]) < dict(CONTIGS)[f[2]] and kept[col], f
        assert f[4] == LETTERS[table[seqs[idx[f[0]], col]]] and f[5] == LETTERS[table[seqs[idx[f[1]], col]]], f
    assert {f[2] for f in rows} == {"chrA", "chrB"}
    # the ruleless run on the alignment the ruled run compared
    plain = os.path.join(td, "compared_sites.csv")
    _cli(monkeypatch, ["pair-sites", "--msa", msa_out, "--pairs", dist, "--filter", "-o", plain])
    back = np.flatnonzero(kept)
    mapped = []
    for f in _read_rows(plain):
        assert f[2] == "alignment"
        col = int(back[int(f[3])])
        contig = "chrA" if col < 2500 else "chrB"
        mapped.append(f[:2] + [contig, str(col - start[contig])] + f[4:])
    assert mapped == rows


@pytest.mark.gpu
def test_a_dropped_sample_is_refused_by_name(hiplib, files, monkeypatch):
    td, fa = files["td"], files["fa"]
    pairs = os.path.join(td, "with_dropped.csv")
    with open(pairs, "w") as fh:
        fh.write("sampleA,sampleB\niso01,iso02\niso03,iso07\n")
    out = os.path.join(td, "with_dropped_sites.csv")
    with pytest.raises(SystemExit) as e:
        _cli(monkeypatch, ["pair-sites", "--msa", fa, "--pairs", pairs, "-o", out, "--max-sample-n-share", "0.25"])
    assert "iso07" in str(e.value) and "--max-sample-n-share" in str(e.value) and "line 3" in str(e.value)
    assert not os.path.exists(out)
    _cli(monkeypatch, ["pair-sites", "--msa", fa, "--pairs", pairs, "-o", out])              # (without the rule the sample is there)
    assert {(f[0], f[1]) for f in _read_rows(out)} == {("iso01", "iso02"), ("iso03", "iso07")}


@pytest.mark.gpu
def test_pairs_across_msa_and_msa_db(hiplib, files, monkeypatch):
    from tracs_amd import synth
    td = files["td"]
    seqs, names = np.array(_seqs()), _names()
    q, db = os.path.join(td, "query.fa"), os.path.join(td, "db.fa")
    synth.write_fasta(q, seqs[:5], names=names[:5])
    synth.write_fasta(db, seqs[5:], names=names[5:])
    pairs = os.path.join(td, "across.csv")
    with open(pairs, "w") as fh:
        fh.write("sampleA,sampleB,anything\niso02,iso20,x\niso20,iso02,x\niso00,iso04,x\niso10,iso11,x\niso02,iso20,x\n")
    out = os.path.join(td, "across_sites.csv")
    _cli(monkeypatch, ["pair-sites", "--msa", q, "--msa-db", db, "--pairs", pairs, "-o", out])
    rows = _read_rows(out)
    masks = _mask_table()[seqs]
    want = []
    for a, b in ((2, 20), (20, 2), (0, 4), (10, 11), (2, 20)):                                 # either order, and a repeat
        for s in np.flatnonzero((masks[a] & masks[b]) == 0):
            want.append([names[a], names[b], "alignment", str(int(s)), LETTERS[masks[a, s]], LETTERS[masks[b, s]], "NA"])
    assert rows == want and len(rows) > 20


# ---- the parser and the error cases: no GPU -------------------------------------------------------------------------------------------
def _pairs_file(tmp_path, text):
    path = os.path.join(str(tmp_path), "pairs.csv")
    with open(path, "w") as fh:
        fh.write(text)
    return path


def test_help_documents_the_command(capsys, monkeypatch):
    with pytest.raises(SystemExit) as e:
        _cli(monkeypatch, ["pair-sites", "-h"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for word in ("--pairs", "--filter", "--max-entries", "--mask-reference", "--max-n-share", "--max-sample-n-share", "--msa-db", "dropped"):
        assert word in text


def test_shared_options_leave_the_distance_parser_as_it_was():
    """the site and sample options are declared once for both commands: same flags, destinations, types and help in `distance`"""
    import argparse
    from tracs_amd.distance import distance_parser
    from tracs_amd.pair_sites import pair_sites_parser
    d = {a.dest: a for a in distance_parser(argparse.ArgumentParser())._actions}
    p = {a.dest: a for a in pair_sites_parser(argparse.ArgumentParser())._actions}
    for dest in ("mask_bed", "keep_bed", "mask_reference", "max_n_share", "max_sample_n_share"):
        for attr in ("option_strings", "type", "default", "metavar", "help"):
            assert getattr(d[dest], attr) == getattr(p[dest], attr), (dest, attr)
    groups = {g.title: [a.dest for a in g._group_actions] for g in distance_parser(argparse.ArgumentParser())._action_groups}
    assert groups["Site selection"] == ["mask_bed", "keep_bed", "mask_reference", "max_n_share", "sites_out"]
    assert groups["Sample and pair selection"] == ["max_sample_n_share", "min_sites", "samples_out"]
    assert p["max_entries"].default == 100000000


def test_unknown_and_ambiguous_names_are_refused_by_name(tmp_path):
    from tracs_amd.pair_sites import read_pairs, resolve_pairs
    path = _pairs_file(tmp_path, "a,b,d\ns1,s2,3\ns3,s1,0\n\ns2,nobody,1\n")
    pairs = read_pairs(path)
    assert pairs == [(2, "s1", "s2"), (3, "s3", "s1"), (5, "s2", "nobody")]
    assert resolve_pairs(pairs[:2], ["s1", "s2", "s3"], path) == ([0, 2], [1, 0])
    with pytest.raises(SystemExit, match=r"line 5: sample 'nobody' is not among the samples"):
        resolve_pairs(pairs, ["s1", "s2", "s3"], path)
    with pytest.raises(SystemExit, match=r"line 5: sample 'nobody' was left out by --max-sample-n-share"):
        resolve_pairs(pairs, ["s1", "s2", "s3"], path, dropped=["nobody"])
    with pytest.raises(SystemExit, match=r"line 2: the name 's2' is carried by two samples"):
        resolve_pairs(pairs, ["s1", "s2", "s3", "s2"], path)
    assert resolve_pairs(pairs[1:2], ["s1", "s2", "s3", "s2"], path) == ([2], [0])            # (an ambiguous name nobody uses is fine)


def test_rows_with_equal_names_or_one_column_are_refused(tmp_path, monkeypatch):
    fa = os.path.join(str(tmp_path), "a.fa")
    with open(fa, "w") as fh:
        fh.write(">s1\nACGT\n>s2\nACGA\n")
    out = os.path.join(str(tmp_path), "out.csv")
    for text, message in (("a,b\ns1,s2\ns2,s2\n", r"line 3: both names are 's2'"), ("a,b\ns1,s2\ns1\n", r"line 3: expected two sample names"),
                          ("a,b\ns1,\n", r"line 2: expected two sample names")):
        pairs = _pairs_file(tmp_path, text)
        with pytest.raises(SystemExit, match=message):
            _cli(monkeypatch, ["pair-sites", "--msa", fa, "--pairs", pairs, "-o", out])
        assert not os.path.exists(out)


def test_more_than_one_msa_is_refused(tmp_path, monkeypatch):
    pairs = _pairs_file(tmp_path, "a,b\ns1,s2\n")
    with pytest.raises(SystemExit, match="give one --msa file"):
        _cli(monkeypatch, ["pair-sites", "--msa", "x.fa", "y.fa", "--pairs", pairs, "-o", os.path.join(str(tmp_path), "o.csv")])


def test_shared_refusals_name_this_command(tmp_path, monkeypatch):
    pairs = _pairs_file(tmp_path, "a,b\ns1,s2\n")
    out = os.path.join(str(tmp_path), "o.csv")
    for extra, message in ((["--max-n-share", "1.5"], r"^tracs pair-sites: --max-n-share must be in \[0, 1\)"),
                           (["--max-sample-n-share", "-1"], r"^tracs pair-sites: --max-sample-n-share must be in \[0, 1\]"),
                           (["--mask-reference", "ref.fa"], r"^tracs pair-sites: --mask-reference needs --mask or --keep")):
        with pytest.raises(SystemExit, match=message):
            _cli(monkeypatch, ["pair-sites", "--msa", "x.fa", "--pairs", pairs, "-o", out] + extra)


def test_max_entries_must_be_a_positive_count(tmp_path, monkeypatch, capsys):
    pairs = _pairs_file(tmp_path, "a,b\ns1,s2\n")
    for bad in ("0", "-3", "many"):
        with pytest.raises(SystemExit) as e:
            _cli(monkeypatch, ["pair-sites", "--msa", "x.fa", "--pairs", pairs, "-o", "o.csv", "--max-entries", bad])
        assert e.value.code == 2
        assert "--max-entries must be a whole number of rows, at least 1, got '%s'" % bad in capsys.readouterr().err


@pytest.mark.gpu
def test_max_entries_refusal_states_the_sum(hiplib, files, monkeypatch):
    td, fa = files["td"], files["fa"]
    pairs = _pairs_file(td, "a,b\niso00,iso01\niso02,iso03\n")
    masks = _mask_table()[_seqs()]
    total = int(((masks[0] & masks[1]) == 0).sum() + ((masks[2] & masks[3]) == 0).sum())
    out = os.path.join(td, "refused.csv")
    with pytest.raises(SystemExit, match=r"tracs pair-sites: the listed pairs differ at %d sites in all, more than --max-entries %d" % (total, total - 1)):
        _cli(monkeypatch, ["pair-sites", "--msa", fa, "--pairs", pairs, "-o", out, "--max-entries", str(total - 1)])
    assert not os.path.exists(out)
    _cli(monkeypatch, ["pair-sites", "--msa", fa, "--pairs", pairs, "-o", out, "--max-entries", str(total)])
    assert len(_read_rows(out)) == total
