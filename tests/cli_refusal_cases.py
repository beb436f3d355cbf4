"""The command lines of tests/test_cli_refusals_pinned.py: every refusal that `tracs distance` and `tracs pair-sites` make before anything
touches the GPU, and pairs of them (which one is reported pins the order of the checks).  tests/golden/make_cli_refusals_golden.py
runs these against a checkout of the commit BEFORE the host layer was refactored and records its texts; nothing here is an expected
value.  Both run in a directory that holds FILES, so every path below is relative to it."""
import argparse
import os

FILES = {
    "two_labels.csv": "sample,group\ns1,a\ns2,b\ns1,b\n",
    "groups.csv": "sample,group\ns1,a\ns2,b\n",
    "reversed.bed": "chr1\t10\t5\n",
    "mask.bed": "chr1\t3\t5\n",
    "long.bed": "chr1\t3\t50\n",
    "dates.csv": "sample,date\ns1,2020-01-01\ns2,2020-01-09\n",
    "pairs.csv": "a,b\ns1,s2\n",
    "x.fa": ">s1\nACGTACGTAC\n>s2\nACGTACGTAA\n",
}

D = ["--msa", "x.fa", "-o", "o.csv"]
P = ["--msa", "x.fa", "--pairs", "pairs.csv", "-o", "o.csv"]
META = ["--meta", "dates.csv"]
ANC = ["--ancestors", "snp"] + META

# (command, argv, what it covers: the line of the refusal in the parent's tracs_amd/distance.py or pair_sites.py)
CASES = [
    # check_ancestors_args
    ("distance", D + ["--ancestors-out", "t.csv"] + META, "distance.py:321"),
    ("distance", D + ANC + ["--mst", "snp"], "distance.py:324"),
    ("distance", D + ANC + ["--nearest", "3"], "distance.py:326"),
    ("distance", D + ANC + ["--histogram"], "distance.py:328 (and :621, which it shadows: the same text)"),
    ("distance", D + ANC + ["--msa-db", "db.fa"], "distance.py:330"),
    ("distance", D + ANC + ["--gpus", "2"], "distance.py:332"),
    ("distance", D + ["--ancestors", "direct"], "distance.py:334"),
    ("distance", D + ["--ancestors", "filter"] + META, "distance.py:336"),
    ("distance", D + ANC + ["--ancestors-out", "dates.csv"], "distance.py:341 (--meta)"),
    ("distance", D + ANC + ["--ancestors-out", "./x.fa"], "distance.py:341 (--msa, another spelling of the path)"),
    ("distance", D + ANC + ["--mask", "mask.bed", "--ancestors-out", "mask.bed"], "distance.py:341 (--mask)"),
    ("distance", D + ANC + ["--ancestors-out", "o.csv"], "distance.py:344 (-o)"),
    ("distance", D + ANC + ["--ancestors-out", "t.fa", "--msa-out", "t.fa"], "distance.py:344 (--msa-out)"),
    ("distance", D + ANC + ["--max-sample-n-share", "0.5", "--samples-out", "s.csv", "--ancestors-out", "s.csv"], "distance.py:344 (--samples-out)"),
    # check_mst_args
    ("distance", D + ["--mst", "snp", "--nearest", "3"], "distance.py:353"),
    ("distance", D + ["--mst", "snp", "--gpus", "2"], "distance.py:355"),
    ("distance", D + ["--mst", "filter"], "distance.py:357"),
    ("distance", D + ["--mst", "direct"], "distance.py:359"),
    ("distance", D + ["--mst", "expectedK", "--filter"], "distance.py:359"),
    # check_histogram_args
    ("distance", D + ["--groups", "groups.csv"], "distance.py:618"),
    ("distance", D + ["--histogram", "--nearest", "3"], "distance.py:623"),
    ("distance", D + ["--histogram", "--mst", "snp"], "distance.py:625"),
    ("distance", D + ["--histogram", "--gpus", "2"], "distance.py:627"),
    ("distance", D + ["--histogram"] + META, "distance.py:629"),
    ("distance", D + ["--histogram", "-K", "3"], "distance.py:631"),
    # check_site_args
    ("distance", D + ["--max-n-share", "1.0"], "distance.py:367"),
    ("distance", D + ["--max-n-share", "nan"], "distance.py:367"),
    ("distance", D + ["--mask-reference", "x.fa"], "distance.py:369"),
    ("distance", D + ["--sites-out", "k.bed"], "distance.py:372"),
    ("distance", D + ["--mask", "mask.bed", "--gpus", "2"], "distance.py:376"),
    ("distance", ["--msa", "x.fa", "y.fa", "-o", "o.csv", "--keep", "mask.bed", "--sites-out", "k.bed"], "distance.py:378"),
    ("distance", D + ["--max-n-share", "0.2", "--sites-out", "k.bed", "--nearest", "3"], "distance.py:380"),
    # check_sample_args
    ("distance", D + ["--max-sample-n-share", "1.5"], "distance.py:455"),
    ("distance", D + ["--min-sites", "0"], "distance.py:457"),
    ("distance", D + ["--samples-out", "s.csv"], "distance.py:459"),
    ("distance", ["--msa", "x.fa", "y.fa", "-o", "o.csv", "--max-sample-n-share", "0.5", "--samples-out", "s.csv"], "distance.py:461"),
    ("distance", D + ["--min-sites", "5", "--gpus", "2"], "distance.py:463"),
    ("distance", D + ["--max-sample-n-share", "0.5", "--gpus", "3"], "distance.py:463"),
    # check_msa_out_args
    ("distance", D + ["--msa-out-sites", "differing"], "distance.py:387"),
    ("distance", D + ["--msa-out", "c.fa", "--msa-db", "db.fa"], "distance.py:391"),
    ("distance", ["--msa", "x.fa", "y.fa", "-o", "o.csv", "--site-table", "t.csv"], "distance.py:393"),
    ("distance", D + ["--msa-out", "c.fa", "--gpus", "2"], "distance.py:395"),
    ("distance", D + ["--msa-out", "x.fa"], "distance.py:401 (--msa-out, --msa)"),
    ("distance", D + ["--histogram", "--groups", "groups.csv", "--site-table", "groups.csv"], "distance.py:401 (--site-table, --groups)"),
    ("distance", D + ["--msa-out", "c.fa", "--site-table", "c.fa"], "distance.py:405"),
    ("distance", D + ["--site-table", "o.csv"], "distance.py:405 (-o)"),
    ("distance", D + ["--mask", "mask.bed", "--sites-out", "o.csv", "--msa-out", "c.fa"], "distance.py:405 (-o and --sites-out)"),
    # read_groups, the BED reader, the bitmap, --nearest with --gpus
    ("distance", D + ["--histogram", "--groups", "two_labels.csv"], "distance.py:648"),
    ("distance", D + ["--mask", "reversed.bed"], "distance.py:534"),
    ("distance", D + ["--nearest", "3", "--gpus", "2"], "distance.py:748"),
    # pair-sites: check_args and the shared checks under its own name
    ("pair-sites", ["--msa", "x.fa", "y.fa", "--pairs", "pairs.csv", "-o", "o.csv"], "pair_sites.py:125"),
    ("pair-sites", P + ["--max-n-share", "1.5"], "pair_sites.py:119 <- distance.py:367"),
    ("pair-sites", P + ["--mask-reference", "x.fa"], "pair_sites.py:119 <- distance.py:369"),
    ("pair-sites", P + ["--max-sample-n-share", "-1"], "pair_sites.py:119 <- distance.py:455"),
    ("pair-sites", ["--msa", "x.fa", "--pairs", "pairs.csv", "-o", "pairs.csv"], "pair_sites.py:131 (--pairs)"),
    ("pair-sites", ["--msa", "x.fa", "--pairs", "pairs.csv", "-o", "x.fa", "--msa-db", "db.fa"], "pair_sites.py:131 (--msa)"),
    ("pair-sites", P + ["--keep", "mask.bed", "-o", "./mask.bed"], "pair_sites.py:131 (--keep)"),
    ("pair-sites", P + ["--mask", "reversed.bed"], "pair_sites.py:119 <- distance.py:534"),
    ("pair-sites", P + ["--mask", "long.bed"], "pair_sites.py:119 <- distance.py:555"),
    # two rules broken at once: the one reported pins the order of the checks
    ("distance", D + ANC + ["--mst", "snp", "--nearest", "3"], "distance.py:324 before :326"),
    ("distance", D + ["--ancestors-out", "t.csv", "--mst", "filter"], "distance.py:321 before :357"),
    ("distance", D + ["--mst", "snp", "--nearest", "2", "--gpus", "2"], "distance.py:353 before :355"),
    ("distance", D + ["--mst", "filter", "--histogram"], "distance.py:357 before :625"),
    ("distance", D + ["--histogram", "--nearest", "3", "--max-n-share", "2"], "distance.py:623 before :367"),
    ("distance", D + ["--histogram", "-K", "2"] + META, "distance.py:629 before :631"),
    ("distance", D + ["--max-n-share", "2", "--max-sample-n-share", "2"], "distance.py:367 before :455"),
    ("distance", D + ["--mask-reference", "x.fa", "--sites-out", "k.bed"], "distance.py:369 before :372"),
    ("distance", D + ["--samples-out", "s.csv", "--min-sites", "0"], "distance.py:457 before :459"),
    ("distance", D + ["--min-sites", "0", "--msa-out-sites", "kept"], "distance.py:457 before :387"),
    ("distance", D + ["--msa-out-sites", "kept", "--nearest", "3", "--gpus", "2"], "distance.py:387 before :748"),
    ("distance", ["--msa", "o.csv", "-o", "o.csv"] + ANC + ["--ancestors-out", "o.csv"], "distance.py:341 before :344"),
    ("distance", D + ["--msa-out", "x.fa", "--site-table", "x.fa"], "distance.py:401 before :405"),
    ("distance", D + ANC + ["--ancestors-out", "c.fa", "--msa-out", "c.fa", "--site-table", "c.fa"], "distance.py:344 before :405"),
    ("distance", D + ["--histogram", "--groups", "two_labels.csv", "--mask", "reversed.bed"], "distance.py:534 before :648"),
    ("distance", D + ["--site-table", "o.csv", "--mask", "reversed.bed"], "distance.py:405 before :534"),
    ("pair-sites", ["--msa", "x.fa", "y.fa", "--pairs", "pairs.csv", "-o", "o.csv", "--max-n-share", "2"], "pair_sites.py:125 before distance.py:367"),
    ("pair-sites", P + ["--max-n-share", "2", "--max-sample-n-share", "2"], "distance.py:367 before :455, as pair-sites"),
    ("pair-sites", ["--msa", "x.fa", "--pairs", "pairs.csv", "-o", "x.fa", "--max-sample-n-share", "2"], "distance.py:455 before pair_sites.py:131"),
    ("pair-sites", ["--msa", "x.fa", "--pairs", "pairs.csv", "-o", "x.fa", "--mask", "reversed.bed"], "pair_sites.py:131 before distance.py:534"),
]

ROUTES = ("nearest_arrays", "pairsnp_arrays", "_rows_on_device", "_forest_on_device", "_histogram_on_device", "_ancestors_on_device")


def write_files(directory):
    for name, text in FILES.items():
        with open(os.path.join(directory, name), "w") as fh:
            fh.write(text)


def refusal(command, argv, replace):
    """Runs `tracs <command> <argv>` in this process, in the current directory (which holds FILES), with every way to the GPU replaced
    by a function that fails (replace(object, name, function)) -> the SystemExit's text with the directory written as {tmp}"""
    import tracs_amd.distance as di
    import tracs_amd.pair_sites as ps
    from tracs_amd import _lib, multigpu

    def no_gpu(*a, **k):
        raise AssertionError("a GPU path was entered or the library was loaded")
    for mod, names in ((multigpu, ("spawn", "init")), (_lib, ("load", "require_gpu")), (di, ROUTES)):
        for name in names:
            replace(mod, name, no_gpu)
    parser = {"distance": di.distance_parser, "pair-sites": ps.pair_sites_parser}[command](argparse.ArgumentParser())
    args = parser.parse_args(argv)
    try:
        args.func(args)
    except SystemExit as e:
        return str(e).replace(os.getcwd(), "{tmp}")
    raise AssertionError("tracs %s %s was not refused" % (command, " ".join(argv)))
