"""`tracs pair-sites` -- the SNP sites behind the pairs of a distance file, with both alleles and the recombination filter's verdict
per SNP (not in the reference).

`tracs distance` reports counts per pair: d, and with --filter a second, smaller one.  This command lists, for the pairs of a CSV
(any `distance` output: the full one, --mst, --nearest), the sites at which the two samples' allele sets are disjoint -- the sites d
counts -- and, with --filter, which of them the filter dropped.  Site and sample rules mean what they mean for `distance`: the run on
the alignment with the dropped columns and records deleted, so under the same rules the rows of a pair number its SNP distance and
the rows with dropped = 0 its filtered distance.  Everything is computed on the GPU (csrc/pair_sites.hip).
"""
import argparse
import ctypes as C
import logging
import os

from . import _lib
from .distance import (_open, add_sample_rule_options, add_site_rule_options, check_output_paths, check_sample_args, check_site_args,
                       read_site_files, site_rule_for)
from .handle import require_files
from .utils import check_positive_int

HEADER = "sampleA,sampleB,contig,position,alleleA,alleleB,dropped\n"
MAX_ENTRIES = 100000000


def check_max_entries(text):
    try:
        v = int(text)
    except ValueError:
        v = 0
    if v < 1:
        raise argparse.ArgumentTypeError("--max-entries must be a whole number of rows, at least 1, got %r" % text)
    return v


def pair_sites_parser(parser):
    parser.description = ("Lists, for each pair of a distance file, the sites at which the two samples differ, with both alleles and "
                          "-- with --filter -- whether the recombination filter dropped the SNP.")
    io = parser.add_argument_group("Input/output")
    io.add_argument("--msa", dest="msa_files", required=True, type=os.path.abspath, nargs="+",
                    help="Input fasta file formatted by the align and merge functions (one file)")
    io.add_argument("--msa-db", dest="msa_db", type=os.path.abspath, default=None,
                    help="A database MSA: pairs may then name samples of either file")
    io.add_argument("--pairs", dest="pairs", required=True, type=os.path.abspath,
                    help="csv with a header line whose first two columns are sample names: any `tracs distance` output (the full "
                         "one, --mst, --nearest).  A pair may be given in either order and may repeat.")
    io.add_argument("-o", "--output", dest="output_file", required=True, type=str,
                    help="name of the output file: sampleA,sampleB,contig,position,alleleA,alleleB,dropped -- one row per site at "
                         "which the two samples' allele sets are disjoint, pairs in the order of --pairs, sites ascending; contig "
                         "and position as `distance --site-table` writes them (0-based, in the coordinates of the input file); "
                         "alleles as upper-case IUPAC letters of the first and the second sample")
    snp = parser.add_argument_group("SNP options")
    snp.add_argument("--filter", dest="recomb_filter", action="store_true", default=False,
                     help="Fill the dropped column: 1 for a SNP that `distance --filter` removes from the pair's filtered SNP "
                          "distance, 0 for one it keeps (without --filter: NA)")
    snp.add_argument("--max-entries", dest="max_entries", type=check_max_entries, default=MAX_ENTRIES, metavar="N",
                     help="Refuse, before anything is written, when the listed pairs have more than N rows in all (default=%d)" % MAX_ENTRIES)
    st = parser.add_argument_group("Site selection",
                                   "As for `distance`: the run on the alignment with the dropped columns deleted from every record. "
                                   "Give the rules of the run that wrote --pairs.")
    add_site_rule_options(st)
    sm = parser.add_argument_group("Sample selection", "As for `distance`: a left-out sample cannot be named in --pairs.")
    add_sample_rule_options(sm)
    parser.add_argument("-t", "--threads", dest="n_cpu", type=check_positive_int, default=1,
                        help="number of threads that format the rows (default=1; the sites are found on the GPU)")
    parser.add_argument("--loglevel", type=str.upper, default="INFO",
                        choices=["DEBUG", "INFO", "WARNING", "ERROR", "CRITICAL"], help="Set the logging threshold.")
    # what the checks shared with `distance` read and this command has no option for
    parser.set_defaults(func=pair_sites, sites_out=None, samples_out=None, min_sites=None, gpus=1, nearest=None)
    return parser


def read_pairs(path):
    """--pairs: csv, header line skipped, the first two columns are sample names -> [(line number, nameA, nameB)] in file order.
    A line without a second column, or with two equal names, is refused with its line number (SystemExit)."""
    out = []
    with open(path, "r") as fh:
        next(fh, None)
        for ln, line in enumerate(fh, 2):
            text = line.rstrip("\r\n")
            if not text.strip():
                continue
            f = text.split(",")
            if len(f) < 2 or not f[0].strip() or not f[1].strip():
                raise SystemExit("tracs pair-sites: %s line %d: expected two sample names in the first two columns, got '%s'" % (path, ln, text))
            a, b = f[0].strip(), f[1].strip()
            if a == b:
                raise SystemExit("tracs pair-sites: %s line %d: both names are '%s' (a pair needs two samples)" % (path, ln, a))
            out.append((ln, a, b))
    return out


def resolve_pairs(pairs, names, path, dropped=()):
    """[(line, nameA, nameB)] -> (rows, cols) index lists into names (the surviving samples).  Refused, naming the sample and the line
    (SystemExit): a name that is not among names (dropped: the names a sample rule left out, for the message), and a name that two
    samples carry."""
    index = {}
    for i, name in enumerate(names):
        index[name] = -1 if name in index else i
    left_out = set(dropped)
    rows, cols = [], []
    for ln, a, b in pairs:
        for name, dst in ((a, rows), (b, cols)):
            i = index.get(name)
            if i is None:
                if name in left_out:
                    raise SystemExit("tracs pair-sites: %s line %d: sample '%s' was left out by --max-sample-n-share" % (path, ln, name))
                raise SystemExit("tracs pair-sites: %s line %d: sample '%s' is not among the samples of the alignment" % (path, ln, name))
            if i < 0:
                raise SystemExit("tracs pair-sites: %s line %d: the name '%s' is carried by two samples" % (path, ln, name))
            dst.append(i)
    return rows, cols


def check_args(args):
    if len(args.msa_files) != 1:
        raise SystemExit("tracs pair-sites: one alignment at a time; give one --msa file")
    check_site_args(args, "pair-sites")
    check_sample_args(args, "pair-sites")
    check_output_paths("pair-sites", {"--msa": args.msa_files[0], "--msa-db": args.msa_db, "--pairs": args.pairs, "--mask": args.mask_bed,
                                      "--keep": args.keep_bed, "--mask-reference": args.mask_reference}, {"-o": args.output_file}, ["-o"])


def pair_sites(args):
    check_args(args)
    site_files = read_site_files(args, "pair-sites")
    pairs = read_pairs(args.pairs)                       # (before anything touches the GPU)
    logging.basicConfig(level=args.loglevel, format="%(asctime)s - %(levelname)s - %(message)s", datefmt="%Y-%m-%d %H:%M:%S")
    msas = [args.msa_files[0], args.msa_db] if args.msa_db is not None else [args.msa_files[0]]
    require_files(msas)
    rule = site_rule_for(msas, args, site_files, "pair-sites")
    _lib.require_gpu()
    logging.info("Reading %s", msas[0])
    with _open(msas, rule, args) as h:
        source = h.source()
        dropped = [name for name, kept in zip(source["source_names"], source["kept"]) if not kept]
        rows, cols = resolve_pairs(pairs, h.names, args.pairs, dropped)
        m = len(rows)
        u32 = C.c_uint32 * max(m, 1)
        contigs = site_files[2]
        nc = len(contigs) if contigs is not None else 0
        cnames = (C.c_char_p * max(nc, 1))(*[c[0].encode() for c in (contigs or [])])
        clens = (C.c_uint64 * max(nc, 1))(*[int(c[1]) for c in (contigs or [])])
        written = C.c_uint64(0)
        logging.info("Listing the SNP sites of %d pairs", m)
        try:
            _lib.check(h.L.tracs_distance_pair_sites(h.h, u32(*rows), u32(*cols), m, int(bool(args.recomb_filter)), int(args.max_entries),
                                                     os.fsencode(args.output_file), cnames, clens, nc, int(args.n_cpu), C.byref(written)))
        except RuntimeError as e:
            raise SystemExit("tracs pair-sites: %s" % e)
        logging.info("Saved %d rows to %s", written.value, args.output_file)


def main():
    parser = pair_sites_parser(argparse.ArgumentParser())
    args = parser.parse_args()
    args.func(args)


if __name__ == "__main__":
    main()
