"""`tracs distance` -- pairwise SNP + transmission distances, GPU path.

Command line, CSV schema and row filtering follow /root/reference/tracs/distance.py:
flags :15-131, dates CSV :145-151, per-MSA pairsnp :159-176, transmission block :179-204,
CSV rows :206-258 (header :157).  The pair loop and the transcluster integral run on the MI355X.
"""
import argparse
import contextlib
import ctypes as C
import logging
import math
import os
import sys
import time
from datetime import date

from . import _lib, switches
from .handle import OPEN_STAGE, DistanceHandle, require_files
from .utils import check_nearest_k, check_positive_float, check_positive_int


def pairsnp_arrays(*args, **kwargs):
    """tracs_amd.api.pairsnp_arrays, imported with numpy on first use (the array route only: --gpus N, incomplete metadata, TRACS_DISTANCE_ARRAYS)"""
    from .api import pairsnp_arrays as f
    return f(*args, **kwargs)


def nearest_arrays(*args, **kwargs):
    """tracs_amd.api.nearest_arrays, imported with numpy on first use (--nearest K)"""
    from .api import nearest_arrays as f
    return f(*args, **kwargs)


def calculate_trans_prob(*args, **kwargs):
    from .transcluster import calculate_trans_prob as f
    return f(*args, **kwargs)

# --mst / --ancestors WEIGHT -> the weight of tracs_distance_forest and tracs_distance_ancestors (the columns `cluster -D` reads: snp 3,
# filter 6, direct 4, expectedK 5); direct (a probability) is read DESCENDING by --ancestors
WEIGHTS = {"snp": 0, "filter": 1, "direct": 2, "expectedK": 3}

ANCESTORS_HEADER = "sample,date,ancestor,ancestor date,root,generation,MSA file\n"

HISTOGRAM_HEADER = "column,distance,within,between,ungrouped,MSA file\n"

TREE_EDGES_HEADER = "parent,child,length,MSA file\n"
TREE_EDGES_SUPPORT_HEADER = "parent,child,length,support,MSA file\n"         # with --bootstrap
TREE_EDGES_TRANSFER_HEADER = "parent,child,length,support,transfer,MSA file\n"      # with --bootstrap-support transfer

TREE_EDGES_CHANGES_HEADER = "parent,child,length,changes,MSA file\n"         # with --tree-changes / --tree-sites
TREE_CHANGES_HEADER = "parent,child,contig,position,alleleParent,alleleChild,MSA file\n"
TREE_SITES_HEADER = "contig,position,changes,minimum,MSA file\n"
TREE_EDGES_FILTER_HEADER = "parent,child,length,changes,filtered,MSA file\n"         # with --tree-filter
TREE_CHANGES_FILTER_HEADER = "parent,child,contig,position,alleleParent,alleleChild,dropped,MSA file\n"

TREE_DISTANCES = {"snp": 0, "per-site": 1}
TREE_METHODS = ("nj", "bionj")                       # --tree METHOD; the second travels as TRACS_TREE_BIONJ in the request's kind

HEADER = ("sampleA,sampleB,date difference,SNP distance,transmission distance,expected K,"
          "filtered SNP distance,sites considered,MSA file\n")


def check_max_entries(text):
    """pair_sites.check_max_entries (that module imports this one)"""
    from .pair_sites import check_max_entries as f
    return f(text)


def add_site_rule_options(st):
    """--mask, --keep, --mask-reference and --max-n-share: the site rules that `distance` and `pair-sites` share"""
    st.add_argument("--mask", dest="mask_bed", default=None, type=os.path.abspath, metavar="BED",
                    help="Columns to drop (BED: 0-based, half-open; alignment columns, or contig coordinates with --mask-reference)")
    st.add_argument("--keep", dest="keep_bed", default=None, type=os.path.abspath, metavar="BED",
                    help="Only these columns may stay.  Together with --mask: keep minus mask.")
    st.add_argument("--mask-reference", dest="mask_reference", default=None, type=os.path.abspath, metavar="REF.fa",
                    help="The reference genome the alignments were made against: contig names and offsets for --mask and --keep "
                         "(columns are its contigs concatenated in file order)")
    st.add_argument("--max-n-share", dest="max_n_share", default=None, type=float, metavar="F",
                    help="Drop a column when more than floor(F n) of the n samples are N there (0 <= F < 1; with --msa-db: the "
                         "samples of both files)")


def add_sample_rule_options(sm):
    """--max-sample-n-share: the sample rule that `distance` and `pair-sites` share"""
    sm.add_argument("--max-sample-n-share", dest="max_sample_n_share", default=None, type=float, metavar="G",
                    help="Leave out a sample when more than floor(G L') of the L' columns that --mask / --keep leave are N in it "
                         "(0 <= G <= 1; 1 drops nothing and only reports; with --msa-db: applied to both files).  --max-n-share then "
                         "counts over the remaining samples.  A left-out sample needs no date in --meta.")


def distance_parser(parser):
    parser.description = ("Estimates pairwise SNP and transmission distances between each pair of samples "
                          "aligned to the same reference genome.")
    io = parser.add_argument_group("Input/output")
    io.add_argument("--msa", dest="msa_files", required=True, type=os.path.abspath, nargs="+",
                    help="Input fasta files formatted by the align and merge functions")
    io.add_argument("--msa-db", dest="msa_db", type=os.path.abspath, default=None,
                    help="A database MSA used to compare each sequence to. By default all pairwise comparisons "
                         "within each MSA are considered.")
    io.add_argument("--meta", dest="metadata", default=None, type=os.path.abspath,
                    help="Location of metadata in csv format. The first column must include the sequence names "
                         "and the second column must include sampling dates.")
    io.add_argument("-o", "--output", dest="output_file", required=True, type=str,
                    help="name of the output file to store the pairwise distance estimates.")
    snp = parser.add_argument_group("SNP distance options")
    snp.add_argument("-D", "--snp_threshold", dest="snp_threshold", type=check_positive_int, default=2147483647,
                     help="Only output those transmission pairs with a SNP distance <= D")
    snp.add_argument("--filter", dest="recomb_filter", action="store_true", default=False,
                     help="Filter out regions with unusually high SNP distances often caused by HGT")
    snp.add_argument("--nearest", dest="nearest", type=check_nearest_k, default=None, metavar="K",
                     help="Only output each sample's K nearest samples (by SNP distance, then input order; 1 <= K <= 1024). "
                          "With --msa-db: the K nearest database samples of each query sample.  Not in the reference.")
    snp.add_argument("--mst", dest="mst", choices=list(WEIGHTS), default=None, metavar="WEIGHT",
                     help="Only output the minimum spanning forest of the pairs the run would write, under the column that "
                          "`cluster -D WEIGHT` reads (snp | filter | direct | expectedK; filter needs --filter, direct and expectedK "
                          "need --meta): at most n - 1 rows, each identical to its row in the full output.  For every threshold T, "
                          "`cluster -c T -D WEIGHT` on this file puts the same samples into the same clusters as on the full file "
                          "(cluster numbers may be permuted).  With --meta every sample needs a date.  Not in the reference.")
    snp.add_argument("--ancestors", dest="ancestors", choices=list(WEIGHTS), default=None, metavar="WEIGHT",
                     help="Only output, for each sample, the pair that links it to its most likely earlier source (SeqTrack-style; "
                          "needs --meta): among the pairs the run would write, the candidates of a sample are its partners with a "
                          "strictly earlier sampling date, and the source is the best of them under (WEIGHT, date gap, input order).  "
                          "WEIGHT: snp | filter | expectedK, smallest first (filter needs --filter), or direct, LARGEST first -- the "
                          "transmission distance column is a probability, so the likeliest source has the largest value (--mst direct "
                          "and `cluster -D direct` read the same column as 'at most a threshold').  At most n - 1 rows, each identical "
                          "to its row in the full output, in pair order.  The file stays a valid `cluster -d` input, but its connected "
                          "components are the transmission trees (the root column of --ancestors-out), not single-linkage clusters.  "
                          "Same-day samples are never linked; a sample without a candidate is a root.  Every compared sample needs a "
                          "date.  One GPU, no --msa-db; not with --mst, --nearest or --histogram.  Not in the reference.")
    snp.add_argument("--ancestors-out", dest="ancestors_out", default=None, type=str, metavar="FILE",
                     help="With --ancestors: write sample,date,ancestor,ancestor date,root,generation,MSA file for every compared "
                          "sample, in input order (dates as --meta gives them; a root has no ancestor, itself as root and generation 0; "
                          "else root is the sample reached by following sources and generation the number of links to it)")
    snp.add_argument("--tree", dest="tree", choices=list(TREE_METHODS), default=None, metavar="METHOD",
                     help="Instead of the pairs, output a phylogeny of each --msa file's samples: nj, the neighbour-joining tree "
                          "(Saitou & Nei) of all pairwise distances, built on the GPU.  -o then holds one Newick tree per --msa file, "
                          "one per line and without a header: unrooted, written from the last node joined, internal nodes unlabelled, "
                          "names quoted where Newick needs it.  Branch lengths are in the unit of --tree-distance; neighbour joining "
                          "can give negative lengths on data that is not tree-like, and they are written as computed.  Ties are "
                          "broken by input order, so the tree is reproducible.  One GPU; takes the site and sample rules, no -D, -K, "
                          "--filter, --meta, --min-sites or --msa-db; not with --nearest, --mst, --ancestors or --histogram.  Not in "
                          "the reference.  bionj: the BIONJ tree (Gascuel 1997), neighbour joining that also keeps the variance of every "
                          "distance (a SNP count's variance grows with the count) and weights each reduction of the matrix to minimise "
                          "the variance of the new row.  It has the same output, options and cost class as nj, about twice its memory, "
                          "and is closer to the true tree when distances are noisy and lineages unequal; every tree of the run "
                          "(--bootstrap replicates, --tree-iterate rebuilds) is then a BIONJ tree.")
    snp.add_argument("--tree-distance", dest="tree_distance", choices=list(TREE_DISTANCES), default=None,
                     help="With --tree: snp (default), the SNP distance; per-site, the SNP distance divided by the sites the pair was "
                          "compared over (substitutions per compared site).  per-site refuses a pair without any compared site: "
                          "leave mostly-N samples out with --max-sample-n-share.")
    snp.add_argument("--tree-edges", dest="tree_edges", default=None, type=str, metavar="FILE",
                     help="With --tree: also write the tree's 2n - 3 edges as parent,child,length,MSA file, in the order they were "
                          "made; internal nodes are named #1, #2, ... by join number, the last one (#(n-2)) joins the remaining three.  "
                          "Sample names are written as they are, as in the other outputs (Newick quotes them)")
    snp.add_argument("--tree-changes", dest="tree_changes", default=None, type=str, metavar="FILE",
                     help="With --tree: place every site of the compared alignment on the tree by small parsimony (Fitch's two passes, "
                          "on the GPU, an IUPAC code read as a set of bases) and write one row per change, "
                          "parent,child,contig,position,alleleParent,alleleChild,MSA file: the SNPs that lie on each branch.  Sites "
                          "ascending, within a site from the top node down; nodes named as in --tree-edges, alleles A/C/G/T, contig and "
                          "position as `pair-sites` and --site-table write them (0-based, in the coordinates of the input file).  The "
                          "NUMBER of changes at a site is its parsimony length on this tree and is unique; their placement on branches is "
                          "one most-parsimonious reconstruction among possibly several (ties go to the parent's base, then A before C "
                          "before G before T).  An N sample never carries a change.  --tree-edges gains a changes column, and one line "
                          "on stderr gives the tree's parsimony length, the sum of the sites' minimum and the consistency index.  Not with "
                          "--bootstrap.  Not in the reference.")
    snp.add_argument("--tree-sites", dest="tree_sites", default=None, type=str, metavar="FILE",
                     help="With --tree: write contig,position,changes,minimum,MSA file for every site with at least one change on the "
                          "tree (see --tree-changes): minimum is the fewest changes any tree needs at the site, and changes - minimum is "
                          "the site's homoplasy -- recombination, hotspots, mapping artefacts.  Not with --bootstrap.")
    snp.add_argument("--max-entries", dest="max_entries", type=check_max_entries, default=None, metavar="N",
                     help="With --tree-changes or --tree-filter: refuse, before anything is written, when the tree has more than N "
                          "changes in all (default=100000000)")
    snp.add_argument("--tree-filter", dest="tree_filter", action="store_true", default=False,
                     help="With --tree and at least one of --tree-edges, --tree-changes, --tree-filtered: run the recombination filter "
                          "of --filter on the changes of every branch (see --tree-changes) instead of on pairs.  A branch's changes are "
                          "what its parent and child states differ by; with d of them in an alignment of L compared sites, a change is "
                          "dropped when the window around it (half width clamp(L / 2d + 1, 50, 5000) sites) holds more changes of that "
                          "branch than a binomial density d / L explains at 0.05 / d.  --tree-edges gains a filtered column (the changes "
                          "kept on the branch) after changes, --tree-changes a dropped column (0 / 1) before MSA file, and one line on "
                          "stderr counts changes, kept, dropped and the branches with a drop.  The tree is still built from the "
                          "UNFILTERED distances: the filter is not iterated into the topology (--tree-iterate does that).  The verdicts belong to the placement "
                          "that --tree-changes writes, one most-parsimonious reconstruction among possibly several.  Not with "
                          "--bootstrap.  Not in the reference.")
    snp.add_argument("--tree-filtered", dest="tree_filtered", default=None, type=str, metavar="FILE",
                     help="With --tree-filter: write one Newick tree per --msa file with the topology and labels of -o and the number "
                          "of changes that --tree-filter keeps on each branch as its length")
    snp.add_argument("--tree-iterate", dest="tree_iterate", default=None, type=int, metavar="K",
                     help="With --tree-filter: iterate the filter into the tree, at most K times (1 <= K <= 100).  The changes that "
                          "--tree-filter drops are masked (set to N) in a copy of the compared alignment, in every sample below their "
                          "branch -- the side of the branch away from the tree's top node, the last node neighbour joining makes --, the "
                          "distances are recomputed, the tree rebuilt and the ORIGINAL alignment placed and filtered on the new tree, "
                          "until the tree has the splits of an earlier one (converged, or a cycle back to an earlier tree) or K trees "
                          "were rebuilt.  -o, --tree-edges, --tree-changes, --tree-sites and --tree-filtered then describe the final "
                          "tree; branch lengths in -o come from the masked distances.  One line on stderr gives the number of trees "
                          "built, how the run ended and the final tree's changes, kept and dropped counts.  The verdicts still belong "
                          "to one Fitch placement among possibly several, and the filter is a screen, not a test: it drops about 13 %% "
                          "of the changes on data without any recombination (DESIGN.md 3.21), so the final tree is built from fewer "
                          "sites than -o without the flag.  Needs a second copy of the alignment on the GPU.  Not with --bootstrap.  "
                          "Not in the reference.")
    snp.add_argument("--tree-iterate-out", dest="tree_iterate_out", default=None, type=str, metavar="FILE",
                     help="With --tree-iterate: write iteration,changes,kept,dropped,branches with a drop,masked cells,shared splits,"
                          "same as,MSA file, one row per tree from the unfiltered one (iteration 0) to the final one: the filter's "
                          "counts on that tree, the cells its verdicts mask (NA on the final row), the splits it shares with the tree "
                          "before (NA on the first row) and, on the final row of a run that ended on a repeat, the iteration whose "
                          "tree it repeats")
    snp.add_argument("--bootstrap", dest="bootstrap", default=None, type=int, metavar="B",
                     help="With --tree: B >= 1 bootstrap replicates, resampled and built on the GPU.  A replicate draws as many columns "
                          "as the run compares, with replacement, and goes through the same distances and the same neighbour joining.  "
                          "Every internal node of the tree in -o is labelled with the NUMBER of replicates, 0 ... B (a count out of B, "
                          "not a percentage), whose tree has the same split of the samples, as in (A:1,B:2)87:0.5; --tree-edges gains a "
                          "support column (NA on the edges to samples).  The result is reproducible bit for bit for a given input, "
                          "rules, B and --bootstrap-seed.  Ties are broken by input order in every replicate, so a group of identical "
                          "samples gets the same arbitrary resolution every time and shows support B: read support only on branches of "
                          "positive length (the edge file has both columns).  Not with --tree-distance per-site.  Not in the reference.")
    snp.add_argument("--bootstrap-support", dest="bootstrap_support", default=None, choices=["split", "transfer"],
                     help="With --bootstrap: what labels the internal nodes.  split (the default): the count described above.  transfer: "
                          "the transfer bootstrap expectation (Lemoine et al. 2018), computed on the GPU.  For a branch and one replicate "
                          "it takes the smallest number of samples that would have to move to turn the branch into some branch of the "
                          "replicate's tree, averages that over the replicates and divides it by the most it can be, the size of the "
                          "branch's lighter side minus one; the label is 1 minus that.  It is a number in [0, 1], not a count: 1 means "
                          "every replicate has the split, and a deep branch that loses one unstable sample in every replicate stays near "
                          "1 where its count is 0.  --tree-edges then has the columns parent,child,length,support,transfer,MSA file (the "
                          "count and the transfer support, both NA on the edges to samples); --bootstrap-trees is unchanged.  As with the "
                          "count, a group of identical samples is resolved the same way in every replicate and shows 1: read the transfer "
                          "support on branches of positive length only.  Not in the reference.")
    snp.add_argument("--bootstrap-seed", dest="bootstrap_seed", default=None, type=int, metavar="S",
                     help="With --bootstrap: the seed of the draws, an integer in [0, 2^64) (default 1)")
    snp.add_argument("--bootstrap-trees", dest="bootstrap_trees", default=None, type=str, metavar="FILE",
                     help="With --bootstrap: also write every replicate's tree, one unlabelled Newick line each, in replicate order "
                          "(the B lines of the first --msa file, then the next file's)")
    snp.add_argument("--histogram", dest="histogram", action="store_true", default=False,
                     help="Instead of the pairs, output how many of them have each SNP distance (and, with --filter, each filtered "
                          "SNP distance): rows column,distance,within,between,ungrouped,MSA file, one per non-empty bin.  The pairs "
                          "are the ones the run would write (-D, --msa-db); they are counted on the GPU and never emitted.  "
                          "`tracs threshold --histogram` reads this file.  Not in the reference.")
    snp.add_argument("--groups", dest="groups", default=None, type=os.path.abspath, metavar="GROUPS.csv",
                     help="With --histogram: csv (header line skipped) of sample name, group label.  A pair counts as `within` when "
                          "both samples have the same label, `between` when they have different labels, `ungrouped` when either has "
                          "none (empty label, or not listed).  Without --groups every pair is `ungrouped`.")
    st = parser.add_argument_group("Site selection",
                                   "A run with a site rule is the run on the alignment with the dropped columns deleted from every "
                                   "record (applied to the packed alignment on the GPU; not in the reference).")
    add_site_rule_options(st)
    st.add_argument("--sites-out", dest="sites_out", default=None, type=str, metavar="FILE",
                    help="Write the kept columns as a BED (readable back through --keep; contig coordinates with --mask-reference)")
    sm = parser.add_argument_group("Sample and pair selection",
                                   "A run with the sample rule is the run on the FASTA file(s) with the dropped records deleted; the pair "
                                   "rule removes pairs from what the run would write (both applied on the GPU; not in the reference).")
    add_sample_rule_options(sm)
    sm.add_argument("--min-sites", dest="min_sites", default=None, type=int, metavar="M",
                    help="Only pairs compared over at least M sites (the `sites considered` column, after the site rules) are eligible: "
                         "for the full output, --nearest, --mst and --histogram alike")
    sm.add_argument("--samples-out", dest="samples_out", default=None, type=str, metavar="FILE",
                    help="With --max-sample-n-share: write sample,MSA file,N sites,sites,kept for every record read, in input order")
    mo = parser.add_argument_group("The compared alignment",
                                   "What the run compared, after every rule: the surviving samples and the kept columns (unpacked and "
                                   "counted on the GPU; not in the reference).  One --msa file, no --msa-db, one GPU.  For the files "
                                   "alone, add --histogram: no pair rows are written.")
    mo.add_argument("--msa-out", dest="msa_out", default=None, type=str, metavar="FILE",
                    help="Write the alignment the run compared as FASTA (gzip when FILE ends in .gz): the surviving samples in order "
                         "under their names, the kept columns, in canonical text -- upper-case IUPAC letters, N for '-' and for every "
                         "byte that is no IUPAC letter.  `distance --msa FILE` without any rule gives the same result.")
    mo.add_argument("--msa-out-sites", dest="msa_out_sites", default=None, choices=["kept", "differing"],
                    help="kept (default): every kept column.  differing: only the columns at which two surviving samples have "
                         "disjoint allele sets -- the columns that add to some SNP distance; every SNP distance stays the same, "
                         "`sites considered` and the filter's alignment length shrink")
    mo.add_argument("--site-table", dest="site_table", default=None, type=str, metavar="FILE",
                    help="Write contig,position,A,C,G,T,N,other,differs per kept column, in order: the surviving samples that are "
                         "exactly that letter, N, or a partial code there, and whether the column differs (positions 0-based, in the "
                         "coordinates of --sites-out)")
    tr = parser.add_argument_group("Transmission distance options")
    tr.add_argument("--clock_rate", dest="clock_rate", type=check_positive_float, default=1e-3 * 29903,
                    help="clock rate as defined in the transcluster paper (SNPs/genome/year) default=1e-3 * 29903")
    tr.add_argument("--trans_rate", dest="trans_rate", type=check_positive_float, default=73.0,
                    help="transmission rate as defined in the transcluster paper (transmissions/year) default=73")
    tr.add_argument("-K", "--trans_threshold", dest="trans_threshold", type=check_positive_int, default=None,
                    help="Only outputs those pairs where the most likely number of intermediate hosts <= K")
    tr.add_argument("--precision", dest="precision", type=check_positive_float, default=0.01,
                    help="The precision used to calculate E(K) (default=0.01).")
    parser.add_argument("-t", "--threads", dest="n_cpu", type=check_positive_int, default=1,
                        help="number of threads to use (default=1; the pair loop runs on the GPU)")
    parser.add_argument("--loglevel", type=str.upper, default="INFO",
                        choices=["DEBUG", "INFO", "WARNING", "ERROR", "CRITICAL"], help="Set the logging threshold.")
    parser.add_argument("--gpus", dest="gpus", type=check_positive_int, default=1,
                        help="number of GPUs of this node to spread the work over (default=1; one process per GPU, each with a slice "
                             "of the sites -- with --filter: with its row panels of the pair matrix --, results gathered on the "
                             "first; not in the reference)")
    parser.set_defaults(func=distance)
    return parser


def _read_dates(path):
    dates = {}
    with open(path, "r") as fh:
        next(fh)                                   # header line is skipped (:148)
        for line in fh:
            f = line.strip().split(",")
            dates[f[0]] = (f[1], date.fromisoformat(f[1]))
    return dates


def _append_rows(path, names, rows, cols, snpd, filt, ncomp, ddiff, tdist, ek, kmax, ref):
    """CSV rows in the reference's format (:206-258), formatted and written by libtracs_hip.so's host code; floats print as
    Python's str(float).  ddiff is None without metadata; filt is None for the "NA" column."""
    import numpy as np
    L = _lib.load()
    u64p, dp = C.POINTER(C.c_uint64), C.POINTER(C.c_double)

    def u64(a):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        return a, a.ctypes.data_as(u64p)

    def f64(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a, a.ctypes.data_as(dp)

    n = len(rows)
    keep = [u64(rows), u64(cols), u64(snpd), u64(ncomp)]
    kf = u64(filt) if filt is not None else (None, None)
    with_dates = ddiff is not None
    fl = [f64(ddiff), f64(tdist), f64(ek)] if with_dates else [(None, None)] * 3
    cnames = (C.c_char_p * len(names))(*[x.encode() for x in names])
    written = C.c_uint64(0)
    _lib.check(L.tracs_write_distance_rows(os.fsencode(path), cnames, keep[0][1], keep[1][1], keep[2][1], kf[1], keep[3][1],
                                           fl[0][1], fl[1][1], fl[2][1], n, int(with_dates),
                                           -1.0 if kmax is None else float(kmax), ref.encode(), C.byref(written)))
    return written.value


class _MissingDate(KeyError):
    """a compared sample that --meta does not list (the full-output route then leaves the alignment to the array route)"""


def ref_of(msa):
    """the `MSA file` column of an alignment's rows (:208-209)"""
    return os.path.basename(msa).split(".")[0].replace("_combined", "")


def _days_of(h, dates, option, metadata=None):
    """The day numbers of the handle's samples, in order, as the c_int32 array the library takes.  A sample without a date:
    SystemExit naming `option` and the metadata file, or -- option None, the full-output route -- _MissingDate."""
    epoch = date(1970, 1, 1)
    got = []
    for name in h.names:
        if name not in dates:
            if option is None:
                raise _MissingDate(name)
            raise SystemExit("tracs distance %s: sample '%s' has no sampling date in %s" % (option, name, metadata))
        got.append((dates[name][1] - epoch).days)
    return (C.c_int32 * max(len(got), 1))(*got)


@contextlib.contextmanager
def _opened(msas, args, stage, rule=None, contigs=None):
    """One alignment's handle for the body of a device-resident route: opened with the rule, its [sum] stage line; after the body
    --msa-out / --site-table from the same handle; freed whatever happens (a body that raises skips those outputs)."""
    with _open(msas, rule, args) as h:
        stage(OPEN_STAGE)
        yield h
        write_msa_outputs(h, args, msas[0], contigs)


def _model_args(h, dates, args, msa, option):
    """What the transmission model of a device route takes from (handle, dates, args): (day numbers, clock rate, transmission rate,
    precision, kmax), with the "Inferring ..." line; without dates: no day numbers, no line, no -K"""
    days, kmax = None, -1.0
    if dates is not None:
        days = _days_of(h, dates, option, args.metadata)
        logging.info("Inferring transmission probabilities for %s", msa)
        kmax = -1.0 if args.trans_threshold is None else float(args.trans_threshold)
    return days, float(args.clock_rate), float(args.trans_rate), float(args.precision), kmax


def _counted(call, h, *head):
    """One tracs_distance_<route> call: the handle, head, then the two counters the library fills -> their values"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    _lib.check(call(h.h, *head, C.byref(a), C.byref(b)))
    return a.value, b.value


def _rows_on_device(msas, args, dates, ref, stage, rule=None, contigs=None):
    """One alignment through libtracs_hip.so's device-resident path (handle.DistanceHandle, tracs_distance_run: include/tracs_hip.h): FASTA -> packed
    planes -> dense panels -> transcluster on the panels -> the pairs within the threshold with their P and E(K) -> ONE device-to-host
    pass, in batches -> the CSV rows, formatted and appended by the library's host threads.  Nothing comes back to Python but the
    sample names (to look the dates up).  -> False when the path does not apply: a sample without a date (the reference raises KeyError
    only if that sample's index is at most the largest index among the emitted pairs, tracs/transcluster.py:23-32: left to the
    array path below, which reproduces that)."""
    try:
        with _opened(msas, args, stage, rule, contigs) as h:
            model = _model_args(h, dates, args, msas[0], None)
            written, pairs = _counted(h.L.tracs_distance_run, h, int(args.snp_threshold), *model, os.fsencode(args.output_file), ref.encode(),
                                      int(bool(args.recomb_filter)))
            stage("[sum] tracs_distance_run (dense panels, transcluster, rows: %d pairs, %d rows written)" % (pairs, written))
    except _MissingDate:
        return False
    return True


def _forest_on_device(msas, args, dates, ref, stage, rule=None, contigs=None):
    """--mst WEIGHT for one alignment (handle.DistanceHandle, tracs_distance_forest: include/tracs_hip.h): the panel walk of _rows_on_device up to the
    pairs within the threshold with their P and E(K), then the minimum spanning forest of the eligible pairs on the device; only its
    rows are formatted and appended.  With metadata every sample needs a date (the full run's array route has KeyError rules of its
    own instead)."""
    with _opened(msas, args, stage, rule, contigs) as h:
        model = _model_args(h, dates, args, msas[0], "--mst")
        written, eligible = _counted(h.L.tracs_distance_forest, h, int(args.snp_threshold), *model, int(bool(args.recomb_filter)),
                                     WEIGHTS[args.mst], os.fsencode(args.output_file), ref.encode())
        stage("[sum] tracs_distance_forest (dense panels, transcluster, forest: %d eligible pairs, %d rows written)" % (eligible, written))


def _ancestors_on_device(msas, args, dates, ref, stage, rule=None, contigs=None):
    """--ancestors WEIGHT for one alignment (handle.DistanceHandle, tracs_distance_ancestors: include/tracs_hip.h): the panel walk of
    _forest_on_device with, instead of the forest, each later-dated sample's best earlier partner kept on the device; only the chosen
    pairs' rows are formatted and appended, and --ancestors-out gets one line per compared sample.  Every compared sample needs a
    date (checked on the opened handle: samples the sample rule left out need none)."""
    with _opened(msas, args, stage, rule, contigs) as h:
        model = _model_args(h, dates, args, msas[0], "--ancestors")
        tree, meta_dates = args.ancestors_out, None
        if tree is not None:
            text = [dates[name][0].encode() for name in h.names]
            meta_dates = (C.c_char_p * max(len(text), 1))(*text)
        written, eligible = _counted(h.L.tracs_distance_ancestors, h, int(args.snp_threshold), *model, int(bool(args.recomb_filter)),
                                     WEIGHTS[args.ancestors], os.fsencode(args.output_file), ref.encode(),
                                     os.fsencode(tree) if tree is not None else None, meta_dates)
        stage("[sum] tracs_distance_ancestors (dense panels, transcluster, ancestors: %d candidates, %d rows written)" % (eligible, written))


def check_output_paths(command, inputs, outputs, own):
    """The path collisions of a run, for its outputs `own` (options of `outputs`).  inputs, outputs: {option: path, list of paths or
    None}.  Refused (SystemExit): an own output that is one of the input files; an own output that names the file of another output
    (a single own option is named in the message)."""
    def real(values):
        return [os.path.realpath(p) for v in values for p in (v if isinstance(v, (list, tuple)) else [v]) if p is not None]
    ins, outs = set(real(inputs.values())), real(outputs.values())
    for opt in own:
        if outputs[opt] is not None and os.path.realpath(outputs[opt]) in ins:
            raise SystemExit("tracs %s: %s %s is one of the run's input files" % (command, opt, outputs[opt]))
    if len(own) == 1:
        if outputs[own[0]] is not None and outs.count(os.path.realpath(outputs[own[0]])) > 1:
            raise SystemExit("tracs %s: %s %s is also another output of the run" % (command, own[0], outputs[own[0]]))
    elif len(set(outs)) != len(outs):
        raise SystemExit("tracs %s: two outputs of the run name the same file" % command)


def _inputs(args):
    return {"--msa": args.msa_files, "--meta": args.metadata, "--mask": args.mask_bed, "--keep": args.keep_bed,
            "--mask-reference": args.mask_reference}


def _outputs(args):
    return {"-o": args.output_file, "--sites-out": args.sites_out, "--samples-out": args.samples_out, "--msa-out": args.msa_out,
            "--site-table": args.site_table}


def check_ancestors_args(args):
    """--ancestors' and --ancestors-out's argument checks, before anything touches the GPU (SystemExit with the message)."""
    anc, out = args.ancestors, args.ancestors_out
    if anc is None:
        if out is not None:
            raise SystemExit("tracs distance: --ancestors-out needs --ancestors (it lists the trees that --ancestors builds)")
        return
    if args.mst is not None:
        raise SystemExit("tracs distance: --ancestors and --mst cannot be combined")
    if args.nearest is not None:
        raise SystemExit("tracs distance: --ancestors and --nearest cannot be combined")
    if args.histogram:
        raise SystemExit("tracs distance: --ancestors and --histogram cannot be combined")
    if args.msa_db is not None:
        raise SystemExit("tracs distance: --ancestors links the samples of one alignment and takes no --msa-db")
    if args.gpus > 1:
        raise SystemExit("tracs distance: --ancestors runs on one GPU; use --gpus 1")
    if args.metadata is None:
        raise SystemExit("tracs distance: --ancestors %s needs --meta (the sampling dates that order the samples)" % anc)
    if anc == "filter" and not args.recomb_filter:
        raise SystemExit("tracs distance: --ancestors filter needs --filter (the filtered SNP distance column)")
    check_output_paths("distance", _inputs(args), dict(_outputs(args), **{"--ancestors-out": out}), ["--ancestors-out"])


def check_tree_args(args):
    """--tree's, --tree-distance's and --tree-edges' argument checks, before anything touches the GPU (SystemExit with the message)."""
    if args.tree is None:
        if args.tree_distance is not None:
            raise SystemExit("tracs distance: --tree-distance needs --tree (it chooses the distances the tree is built from)")
        if args.tree_edges is not None:
            raise SystemExit("tracs distance: --tree-edges needs --tree (it lists the edges of the tree that --tree builds)")
        for opt, value in (("--bootstrap", args.bootstrap), ("--bootstrap-seed", args.bootstrap_seed), ("--bootstrap-trees", args.bootstrap_trees)):
            if value is not None:
                raise SystemExit("tracs distance: %s needs --tree (it resamples the alignment that --tree builds its tree from)" % opt)
        if args.bootstrap_support is not None:
            raise SystemExit("tracs distance: --bootstrap-support needs --bootstrap, which needs --tree (it chooses what the replicates' trees "
                             "say about the branches of the tree that --tree builds)")
        for opt, value in (("--tree-changes", args.tree_changes), ("--tree-sites", args.tree_sites)):
            if value is not None:
                raise SystemExit("tracs distance: %s needs --tree (it places the sites on the tree that --tree builds)" % opt)
        if args.max_entries is not None:
            raise SystemExit("tracs distance: --max-entries needs --tree-changes, which needs --tree (it bounds the rows of that file)")
        if args.tree_filter:
            raise SystemExit("tracs distance: --tree-filter needs --tree (it filters the changes on the branches of the tree that --tree builds)")
        if args.tree_iterate is not None or args.tree_iterate_out is not None:
            raise SystemExit("tracs distance: --tree-iterate needs --tree-filter, which needs --tree (it rebuilds the tree that --tree builds "
                             "without the changes that --tree-filter drops)")
        if args.tree_filtered is not None:
            raise SystemExit("tracs distance: --tree-filtered needs --tree-filter, which needs --tree (it holds the tree with the kept changes "
                             "as branch lengths)")
        return
    for opt, given in (("--nearest", args.nearest is not None), ("--mst", args.mst is not None),
                       ("--ancestors", args.ancestors is not None), ("--histogram", args.histogram)):
        if given:
            raise SystemExit("tracs distance: --tree and %s cannot be combined" % opt)
    if args.snp_threshold != 2147483647:
        raise SystemExit("tracs distance: --tree joins all samples and takes no -D (every pair's distance is used)")
    if args.trans_threshold is not None:
        raise SystemExit("tracs distance: --tree is built from SNP distances and takes no -K")
    if args.recomb_filter:
        raise SystemExit("tracs distance: --tree is built from the unfiltered SNP distances and takes no --filter")
    if args.metadata is not None:
        raise SystemExit("tracs distance: --tree is built from SNP distances and takes no --meta")
    if args.min_sites is not None:
        raise SystemExit("tracs distance: --tree needs every pair's distance and takes no --min-sites (use --max-sample-n-share)")
    if args.msa_db is not None:
        raise SystemExit("tracs distance: --tree joins the samples of one alignment and takes no --msa-db")
    if args.gpus > 1:
        raise SystemExit("tracs distance: --tree runs on one GPU; use --gpus 1")
    if args.bootstrap is None:
        for opt, value in (("--bootstrap-seed", args.bootstrap_seed), ("--bootstrap-trees", args.bootstrap_trees),
                           ("--bootstrap-support", args.bootstrap_support)):
            if value is not None:
                raise SystemExit("tracs distance: %s needs --bootstrap (it belongs to the replicates that --bootstrap draws)" % opt)
    else:
        if not 1 <= args.bootstrap < 2 ** 32:
            raise SystemExit("tracs distance: --bootstrap %d: the number of replicates must be at least 1 (and below 2^32)" % args.bootstrap)
        if args.bootstrap_seed is not None and not 0 <= args.bootstrap_seed < 2 ** 64:
            raise SystemExit("tracs distance: --bootstrap-seed %d is outside [0, 2^64)" % args.bootstrap_seed)
        if TREE_DISTANCES[args.tree_distance or "snp"] == 1:
            raise SystemExit("tracs distance: --bootstrap resamples SNP distances and takes no --tree-distance per-site (a replicate's "
                             "compared-site counts need every column, not only the differing ones)")
    for opt, given in (("--tree-changes", args.tree_changes is not None), ("--tree-sites", args.tree_sites is not None),
                       ("--tree-filter", args.tree_filter)):
        if given and args.bootstrap is not None:
            raise SystemExit("tracs distance: %s and --bootstrap cannot be combined yet (the tree is reproducible bit for bit: run once with "
                             "each and join the two --tree-edges files on parent and child)" % opt)
    if args.tree_filtered is not None and not args.tree_filter:
        raise SystemExit("tracs distance: --tree-filtered needs --tree-filter (it holds the tree with the kept changes as branch lengths)")
    if args.tree_iterate is None:
        if args.tree_iterate_out is not None:
            raise SystemExit("tracs distance: --tree-iterate-out needs --tree-iterate (it lists the trees that --tree-iterate builds)")
    else:
        if args.bootstrap is not None:
            raise SystemExit("tracs distance: --tree-iterate and --bootstrap cannot be combined (the replicates would have to be drawn from "
                             "the masked alignment of the final tree)")
        if not args.tree_filter:
            raise SystemExit("tracs distance: --tree-iterate needs --tree-filter (it masks the changes that --tree-filter drops)")
        if not 1 <= args.tree_iterate <= 100:
            raise SystemExit("tracs distance: --tree-iterate %d: the number of iterations must be in [1, 100]" % args.tree_iterate)
    if args.tree_filter and args.tree_edges is None and args.tree_changes is None and args.tree_filtered is None:
        raise SystemExit("tracs distance: --tree-filter needs --tree-edges, --tree-changes or --tree-filtered (the files its verdicts go to)")
    if args.max_entries is not None and args.tree_changes is None and not args.tree_filter:
        raise SystemExit("tracs distance: --max-entries needs --tree-changes (it bounds the rows of that file; --tree-sites has at most one "
                         "row per site)")
    check_output_paths("distance", _inputs(args), dict(_outputs(args), **{"--tree-edges": args.tree_edges}), ["--tree-edges"])
    tree_outputs = dict(_outputs(args), **{"--tree-edges": args.tree_edges, "--tree-changes": args.tree_changes, "--tree-sites": args.tree_sites})
    check_output_paths("distance", _inputs(args), tree_outputs, ["--tree-changes"])
    check_output_paths("distance", _inputs(args), tree_outputs, ["--tree-sites"])
    check_output_paths("distance", _inputs(args), dict(_outputs(args), **{"--tree-edges": args.tree_edges, "--bootstrap-trees": args.bootstrap_trees}),
                       ["--bootstrap-trees"])
    if args.tree_filtered is not None:
        check_output_paths("distance", _inputs(args), dict(tree_outputs, **{"--tree-filtered": args.tree_filtered}), ["--tree-filtered"])
    if args.tree_iterate_out is not None:
        check_output_paths("distance", _inputs(args), dict(tree_outputs, **{"--tree-filtered": args.tree_filtered,
                                                                            "--tree-iterate-out": args.tree_iterate_out}), ["--tree-iterate-out"])


def tree_changes_on(args):
    """the run places the sites on the tree (the changes stage of the tree request): the library then creates the run's files itself"""
    return args.tree is not None and (args.tree_changes is not None or args.tree_sites is not None or args.tree_filter)


def tree_edges_header(args):
    """the header of --tree-edges for what the run asks of the tree"""
    return (TREE_EDGES_FILTER_HEADER if args.tree_filter else TREE_EDGES_CHANGES_HEADER if tree_changes_on(args) else
            TREE_EDGES_HEADER if args.bootstrap is None else
            TREE_EDGES_TRANSFER_HEADER if args.bootstrap_support == "transfer" else TREE_EDGES_SUPPORT_HEADER)


def _tree_on_device(msas, args, dates, ref, stage, rule=None, contigs=None, tree_contigs=None):
    """--tree nj / bionj for one alignment (handle.DistanceHandle.tree, tracs_distance_tree_run: include/tracs_hip.h): every dense panel goes into
    the distance matrix on the device, the joins run there, and one Newick line (and the edge rows) are appended by the library."""
    changes_on = tree_changes_on(args)
    # (the [sum] lines name the method; nj's stay as they were)
    named = stage if args.tree == "nj" else lambda line: stage("%s [%s]" % (line, args.tree))
    with _opened(msas, args, stage, rule, contigs) as h:
        try:
            # (the changes stage: the library creates the files itself, once the count has passed --max-entries: a refusal touches nothing)
            t = h.tree(args.output_file, ref, per_site=TREE_DISTANCES[args.tree_distance or "snp"] == 1, edges_path=args.tree_edges,
                       bootstrap=args.bootstrap or 0, seed=1 if args.bootstrap_seed is None else args.bootstrap_seed,
                       replicate_trees=args.bootstrap_trees, support=args.bootstrap_support or "split", changes_path=args.tree_changes,
                       sites_path=args.tree_sites, max_entries=args.max_entries, contigs=tree_contigs, n_threads=args.n_cpu,
                       create=not args.tree_files_made, tree_filter=args.tree_filter, filtered_path=args.tree_filtered,
                       **({} if args.tree_iterate is None else {"iterate": args.tree_iterate, "iterations_path": args.tree_iterate_out}),
                       **({} if args.tree == "nj" else {"method": args.tree}))
        except RuntimeError as e:
            if not changes_on:                                              # (the plain and the bootstrap run pass the library's error on)
                raise
            raise SystemExit("tracs distance: %s" % e)
        args.tree_files_made = True                                        # (read by the changes stage only)
        if args.tree_changes is not None or args.tree_sites is not None:
            sys.stderr.write("tracs distance: %s: parsimony length %d, minimum %d, consistency index %s\n"
                             % (ref, t.changes, t.minimum, repr(t.minimum / t.changes) if t.changes else "1"))
        if args.tree_filter:
            sys.stderr.write("tracs distance: %s: tree filter: %d changes, %d kept, %d dropped, %d branches with a drop\n"
                             % (ref, t.changes, t.kept, t.changes - t.kept, t.branches))
            if args.tree_iterate is not None:
                how = ("stopped at the limit" if t.same_as is None else "converged" if t.same_as == t.iterations - 1 else
                       "cycle back to %d" % t.same_as)
                sys.stderr.write("tracs distance: %s: tree iterate: %d trees built, %s; final tree: %d changes, %d kept, %d dropped\n"
                                 % (ref, t.iterations + 1, how, t.changes, t.kept, t.changes - t.kept))
                named("[sum] tracs_distance_tree_iterate (%d trees: dense panels, joins, Fitch count, edge lists, filter, mask each; tree, fill: "
                      "%d joins, %d edge rows, %d changes, %d kept)" % (t.iterations + 1, t.joins, t.rows, t.changes, t.kept))
            else:
                named("[sum] tracs_distance_tree_filter (dense panels, joins, tree, Fitch count, edge lists, filter, fill: %d joins, %d edge rows, "
                      "%d changes, %d kept)" % (t.joins, t.rows, t.changes, t.kept))
        elif changes_on:
            named("[sum] tracs_distance_tree_changes (dense panels, joins, tree, Fitch count and fill: %d joins, %d edge rows, %d changes)"
                  % (t.joins, t.rows, t.changes))
        elif args.bootstrap is not None:
            named("[sum] tracs_distance_tree_bootstrap%s (main tree, %d replicates: %d joins, %d edge rows written)"
                  % ("_transfer" if args.bootstrap_support == "transfer" else "", args.bootstrap, t.joins, t.rows))
        else:
            named("[sum] tracs_distance_tree (dense panels, joins, tree: %d joins, %d edge rows written)" % (t.joins, t.rows))


def check_mst_args(args):
    """--mst's argument checks, before anything touches the GPU (SystemExit with the message)."""
    mst = args.mst
    if mst is None:
        return
    if args.nearest is not None:
        raise SystemExit("tracs distance: --mst and --nearest cannot be combined")
    if args.gpus > 1:
        raise SystemExit("tracs distance: --mst runs on one GPU; use --gpus 1")
    if mst == "filter" and not args.recomb_filter:
        raise SystemExit("tracs distance: --mst filter needs --filter (the filtered SNP distance column)")
    if mst in ("direct", "expectedK") and args.metadata is None:
        raise SystemExit("tracs distance: --mst %s needs --meta (the sampling dates that transmission distances come from)" % mst)


def check_site_args(args, command="distance"):
    """The site rules' argument checks, before anything touches the GPU (SystemExit with the message, under the command's name)."""
    mask, keep, share, ref, out = args.mask_bed, args.keep_bed, args.max_n_share, args.mask_reference, args.sites_out
    if share is not None and not (0.0 <= share < 1.0):            # (a NaN fails too)
        raise SystemExit("tracs %s: --max-n-share must be in [0, 1), got %r" % (command, share))
    if ref is not None and mask is None and keep is None:
        raise SystemExit("tracs %s: --mask-reference needs --mask or --keep (it only gives their contigs an offset)" % command)
    rule = mask is not None or keep is not None or share is not None
    if out is not None and not rule:
        raise SystemExit("tracs %s: --sites-out needs a site rule (--mask, --keep or --max-n-share)" % command)
    if not rule:
        return
    if args.gpus > 1:
        raise SystemExit("tracs %s: site rules (--mask, --keep, --max-n-share) run on one GPU; use --gpus 1" % command)
    if out is not None and len(args.msa_files) > 1:
        raise SystemExit("tracs %s: --sites-out describes one alignment; give one --msa file" % command)
    if out is not None and share is not None and args.nearest is not None:
        raise SystemExit("tracs %s: --sites-out with --nearest takes file rules only (--mask, --keep), not --max-n-share" % command)


def check_msa_out_args(args):
    """--msa-out / --msa-out-sites / --site-table: argument checks, before anything touches the GPU (SystemExit with the message)."""
    out, which, table = args.msa_out, args.msa_out_sites, args.site_table
    if which is not None and out is None:
        raise SystemExit("tracs distance: --msa-out-sites needs --msa-out (it chooses the columns of that file)")
    if out is None and table is None:
        return
    if args.msa_db is not None:
        raise SystemExit("tracs distance: --msa-out and --site-table describe one alignment and take no --msa-db")
    if len(args.msa_files) > 1:
        raise SystemExit("tracs distance: --msa-out and --site-table describe one alignment; give one --msa file")
    if args.gpus > 1:
        raise SystemExit("tracs distance: --msa-out and --site-table run on one GPU; use --gpus 1")
    check_output_paths("distance", dict(_inputs(args), **{"--groups": args.groups}), _outputs(args), ["--msa-out", "--site-table"])


def write_msa_outputs(h, args, msa, contigs):
    """--msa-out and --site-table for what the handle compares (the surviving samples, the kept columns): the census and the unpack
    run on the GPU (tracs_distance_site_census / _write_alignment), one INFO line per file.  The handle is left as it was."""
    out, table = args.msa_out, args.site_table
    if out is None and table is None:
        return
    import numpy as np
    from . import sites as S
    L, n, length = h.L, h.n, h.length
    counts = np.zeros((6, length), np.uint32) if table is not None else None
    differs = np.zeros((length + 63) // 64, np.uint64)
    n_differs = C.c_size_t(0)
    _lib.check(L.tracs_distance_site_census(h.h, counts.ctypes.data if counts is not None else None,
                                            differs.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n_differs)))
    if table is not None:
        S.write_site_table(table, h.kept_positions(), counts, S.bitmap_to_bool(differs, length), contigs)
        logging.info("Site table for %s: %s (%d samples, %d columns, %d differing)", msa, table, n, length, n_differs.value)
    if out is not None:
        written = C.c_size_t(0)
        _lib.check(L.tracs_distance_write_alignment(h.h, os.fsencode(out), 0, n, int(args.msa_out_sites == "differing"), int(args.n_cpu), -1,
                                                    C.byref(written)))
        logging.info("Compared alignment of %s: %s (%d records, %d columns, %d differing)", msa, out, n, written.value, n_differs.value)


def _msa_outputs_fresh(msas, args, rule, contigs):
    """write_msa_outputs for the routes without a distance handle: one is opened with the same rules for the write"""
    if args.msa_out is None and args.site_table is None:
        return
    with _open(msas, rule, args) as h:
        write_msa_outputs(h, args, msas[0], contigs)


SAMPLES_HEADER = "sample,MSA file,N sites,sites,kept\n"


def check_sample_args(args, command="distance"):
    """The sample and pair rules' argument checks, before anything touches the GPU (SystemExit with the message, under the command's
    name)."""
    share, m, out = args.max_sample_n_share, args.min_sites, args.samples_out
    if share is not None and not (0.0 <= share <= 1.0):            # (a NaN fails too)
        raise SystemExit("tracs %s: --max-sample-n-share must be in [0, 1], got %r" % (command, share))
    if m is not None and not (1 <= m <= 0xFFFFFFFF):
        raise SystemExit("tracs %s: --min-sites must be in [1, 2^32 - 1], got %r" % (command, m))
    if out is not None and share is None:
        raise SystemExit("tracs %s: --samples-out needs --max-sample-n-share (it lists what the sample rule decided)" % command)
    if out is not None and len(args.msa_files) > 1:
        raise SystemExit("tracs %s: --samples-out describes one alignment; give one --msa file" % command)
    if (share is not None or m is not None) and args.gpus > 1:
        raise SystemExit("tracs %s: the sample and pair rules (--max-sample-n-share, --min-sites) run on one GPU; use --gpus 1" % command)


def write_samples_out(path, names, ref, n_counts, sites, kept):
    """--samples-out: one row per record read, in input order: sample,MSA file,N sites,sites,kept (kept: 1 or 0)"""
    with open(path, "w") as fh:
        fh.write(SAMPLES_HEADER)
        for name, cnt, k in zip(names, n_counts, kept):
            fh.write("%s,%s,%d,%d,%d\n" % (name, ref, int(cnt), int(sites), 1 if k else 0))


class _SiteRule:
    """The rules of one alignment, as the keywords of the library's FASTA entry points.  Site rules: the keep bitmap over its columns
    (None: files give none) and the N rule, as a threshold max_n (None: none) or -- with the sample rule (sample_share) or the pair rule
    (min_sites), because it then counts over the samples that survive -- as its share."""

    def __init__(self, L, keep, max_n, contigs, share=None, sample_share=None, min_sites=None):
        from .sites import Sites
        self.L, self.keep, self.max_n, self.contigs = L, keep, max_n, contigs
        self.share, self.sample_share, self.min_sites = share, sample_share, min_sites
        self.sites = Sites(keep, max_n)
        self.reported = False

    def has_site_rule(self):
        return self.keep is not None or self.max_n is not None or self.share is not None

    def rules(self):
        """what handle.rules_struct (DistanceHandle) takes for this rule"""
        return dict(sites=self.sites, max_sample_n_share=self.sample_share, max_n_share=self.share, min_sites=self.min_sites)

    def api_kwargs(self, info):
        """what pairsnp_arrays / nearest_arrays take for this rule: the rule keywords only with the sample or the pair rule"""
        if self.sample_share is None and self.min_sites is None:
            return dict(sites=self.sites, info=info)
        return dict(self.rules(), info=info)

    def report(self, args, msa, kept_words=None, n_kept=None, source=None):
        """the INFO lines of the alignment, --sites-out and --samples-out, once.  source: what the sample rule saw
        (handle.source_records), with the sample rule"""
        from . import sites as S
        if self.reported:
            return
        self.reported = True
        if self.sample_share is not None and source is not None:
            names, kept, rule_sites = source["source_names"], source["kept"], source["rule_sites"]
            logging.info("Sample rule for %s: kept %d of %d samples (dropped: N at more than %d of %d columns)", msa, int(sum(bool(k) for k in kept)),
                         len(names), math.floor(self.sample_share * rule_sites), rule_sites)
            if args.samples_out is not None:
                write_samples_out(args.samples_out, names, ref_of(msa), source["n_counts"], rule_sites, kept)
        if not self.has_site_rule():
            return
        by_files = self.L - int(self.keep.sum()) if self.keep is not None else 0
        if n_kept is None:
            n_kept = int(S.bitmap_to_bool(kept_words, self.L).sum())
        logging.info("Site rules for %s: kept %d of %d columns (%d dropped by --mask / --keep, %d by --max-n-share)",
                     msa, n_kept, self.L, by_files, self.L - by_files - n_kept)
        if args.sites_out is not None:
            S.write_kept_bed(args.sites_out, kept_words if kept_words is not None else self.keep, self.L, self.contigs)


def read_site_files(args, command="distance"):
    """--mask / --keep / --mask-reference, read once: (keep intervals or None, mask intervals or None, contigs or None); ValueError ->
    SystemExit with the message"""
    from . import sites as S
    contigs = None
    try:
        if args.mask_reference is not None:
            from .align_post import read_contigs
            contigs = read_contigs(args.mask_reference)
        keep = S.read_bed(args.keep_bed, contigs) if args.keep_bed is not None else None
        mask = S.read_bed(args.mask_bed, contigs) if args.mask_bed is not None else None
    except ValueError as e:
        raise SystemExit("tracs %s: %s" % (command, e))
    return keep, mask, contigs


def site_rule_for(msas, args, files, command="distance"):
    """The rule of one alignment (None without any site option).  The bitmap needs the alignment's length and the share the number of
    loaded samples before the library opens the files: the length comes from the first record; the sample count, only with
    --max-n-share, from a host-side read of the files (the library's own FASTA reader)."""
    from . import sites as S
    keep_iv, mask_iv, contigs = files
    share, sample_share, min_sites = args.max_n_share, args.max_sample_n_share, args.min_sites
    if keep_iv is None and mask_iv is None and share is None and sample_share is None and min_sites is None:
        return None
    require_files(msas)
    L = S.first_record_length(msas[0]) if (keep_iv is not None or mask_iv is not None or share is not None) else 0      # (0: no site rule)
    keep = None
    if keep_iv is not None or mask_iv is not None:
        try:
            keep = S.keep_bool(L, keep_iv, mask_iv)
        except ValueError as e:
            raise SystemExit("tracs %s: %s: %s" % (command, msas[0], e))
    max_n = None
    if sample_share is not None or min_sites is not None:
        # the library takes F itself and computes floor(F n') over the samples that survive the sample rule: no host read for n
        return _SiteRule(L, keep, None, contigs, share=share, sample_share=sample_share, min_sites=min_sites)
    if share is not None:
        lib = _lib.load()
        n = 0
        for p in msas:
            cnt, length = C.c_size_t(0), C.c_size_t(0)
            _lib.check(lib.tracs_debug_read_fasta(os.fsencode(p), C.byref(cnt), C.byref(length), None))
            n += cnt.value
        max_n = S.max_n_samples(share, n)
    return _SiteRule(L, keep, max_n, contigs)


@contextlib.contextmanager
def _open(msas, rule, args):
    """The alignment's handle, opened with the rule; with one: its INFO lines, --sites-out and --samples-out before the body"""
    with DistanceHandle(msas, **(rule.rules() if rule is not None else {})) as h:
        if rule is not None:
            rule.L = h.source_len
            rule.report(args, msas[0], kept_words=h.kept_words(), n_kept=h.length, source=h.source() if rule.sample_share is not None else None)
        yield h


def _report_arrays(rule, args, msa, info):
    """rule.report for the array routes: what pairsnp_arrays / nearest_arrays left in `info`"""
    rule.report(args, msa, n_kept=info["seqlen"], source=info if "source_names" in info else None)


def check_histogram_args(args):
    """--histogram's and --groups' argument checks, before anything touches the GPU (SystemExit with the message)."""
    if not args.histogram:
        if args.groups is not None:
            raise SystemExit("tracs distance: --groups needs --histogram (the labels only split the histogram's counts)")
        return
    if args.ancestors is not None:
        raise SystemExit("tracs distance: --ancestors and --histogram cannot be combined")
    if args.nearest is not None:
        raise SystemExit("tracs distance: --histogram and --nearest cannot be combined")
    if args.mst is not None:
        raise SystemExit("tracs distance: --histogram and --mst cannot be combined")
    if args.gpus > 1:
        raise SystemExit("tracs distance: --histogram runs on one GPU; use --gpus 1")
    if args.metadata is not None:
        raise SystemExit("tracs distance: --histogram counts SNP distances and takes no --meta (no histogram of transmission distances)")
    if args.trans_threshold is not None:
        raise SystemExit("tracs distance: --histogram counts SNP distances and takes no -K (no histogram of E(K))")


def read_groups(path):
    """--groups: csv, header line skipped (as --meta, :148), first column the sample name, second the group label.  -> {name: label};
    an empty label (or a line without a second column) leaves the sample ungrouped; one name with two different labels is an error."""
    groups = {}
    with open(path, "r") as fh:
        next(fh, None)
        for line in fh:
            f = line.rstrip("\r\n").split(",")
            name = f[0].strip()
            if not name:
                continue
            label = f[1].strip() if len(f) > 1 else ""
            label = label if label else None
            if name in groups and groups[name] != label:
                raise SystemExit("tracs distance: --groups %s lists sample '%s' with two different labels ('%s' and '%s')"
                                 % (path, name, "" if groups[name] is None else groups[name], "" if label is None else label))
            groups[name] = label
    return groups


def _histogram_on_device(msas, args, groups, ref, stage, rule=None, contigs=None):
    """--histogram for one alignment (handle.DistanceHandle, tracs_distance_histogram: include/tracs_hip.h): the panel walk of _rows_on_device with
    a histogram update per panel instead of the rows; only the non-empty bins are formatted and appended."""
    from .api import group_labels
    with _opened(msas, args, stage, rule, contigs) as h:
        labels = None
        if groups is not None:
            names = h.names
            n = len(names)
            lab = group_labels(names, groups)
            labels = (C.c_int32 * max(n, 1))(*[int(x) for x in lab])
            logging.info("%d of %d samples of %s have a group label (%d groups)", int((lab >= 0).sum()), n, msas[0],
                         int(lab.max()) + 1 if n else 0)
        eligible, written = _counted(h.L.tracs_distance_histogram, h, int(args.snp_threshold), int(bool(args.recomb_filter)), labels,
                                     os.fsencode(args.output_file), ref.encode())
        stage("[sum] tracs_distance_histogram (dense panels, histogram: %d pairs counted, %d rows written)" % (eligible, written))


def _cli_of(args):
    """The command line that reproduces `args` (the multi-GPU path re-launches itself, one process per GPU)."""
    argv = ["distance", "--msa"] + list(args.msa_files) + ["-o", args.output_file, "-D", str(args.snp_threshold),
                                                            "--clock_rate", repr(float(args.clock_rate)), "--trans_rate", repr(float(args.trans_rate)),
                                                            "--precision", repr(float(args.precision)), "-t", str(args.n_cpu),
                                                            "--loglevel", args.loglevel, "--gpus", str(args.gpus)]
    if args.msa_db is not None:
        argv += ["--msa-db", args.msa_db]
    if args.metadata is not None:
        argv += ["--meta", args.metadata]
    if args.recomb_filter:
        argv += ["--filter"]
    if args.trans_threshold is not None:
        argv += ["-K", str(args.trans_threshold)]
    return argv


def _pairs_multi_gpu(msas, args, ctx):
    """pairsnp's six outputs for one MSA, computed by all ranks and assembled on rank 0 (None on the others)."""
    import numpy as np
    from . import device as dev
    from . import multigpu, partition
    dist, rank, world, device = ctx
    if not args.recomb_filter and switches.get("TRACS_DIST_PARTITION", "sites") == "sites":
        # SITE shards (the default): every rank holds 1 / P of the sites and counts all pairs over them -- every stage of the call,
        # what is built once per alignment included, works on 1 / P of the data; the sums arrive as row panels (reduce-scatter)
        aln = multigpu.site_sharded_alignment(msas, dist, rank, world, device)
        n = aln.n
        i_end, j_start = (n, 0) if len(msas) == 1 else (aln.n_first, aln.n_first)      # src/pairsnp.hpp:348-360
        got = multigpu.pairs_site_sharded(aln, i_end, j_start, args.snp_threshold, rank, world, dist)
        names = aln.names
        aln.close()
        if rank != 0:
            return None
        host = [g.cpu().numpy().astype(np.uint32).astype(np.uint64) for g in got]
        return host[0], host[1], host[2], names, np.zeros(len(host[0]), np.uint64), host[3]      # filter off: `len` zeros (:452)
    # PAIR partition (with --filter: the recombination filter wants every site of a pair in one place): every rank holds the whole
    # alignment and computes its row panels
    if switches.get("TRACS_DIST_PARSE_ALL"):
        aln = dev.Alignment.from_fasta(msas)              # every rank parses and packs
    else:
        aln = multigpu.shared_alignment(msas, dist, rank, world, device)      # rank 0 parses, the packed planes are broadcast
    n = aln.n
    i_end, j_start = (n, 0) if len(msas) == 1 else (aln.n_first, aln.n_first)      # src/pairsnp.hpp:348-360
    parts = multigpu.pairs_of_rank(aln, i_end, j_start, args.snp_threshold, rank, world, args.recomb_filter)
    got = partition.gather_coo(parts, world, rank, dist)
    names = aln.names
    aln.close()
    if rank != 0:
        return None
    host = [g.cpu().numpy().astype(np.uint32).astype(np.uint64) for g in got]
    filt = host[4] if args.recomb_filter else np.zeros(len(host[0]), np.uint64)     # filter off: `len` zeros (:452)
    return host[0], host[1], host[2], names, filt, host[3]


class _Stages:
    """The "[stage] name seconds" lines on stderr under TRACS_STAGE_TRACE (scripts/bench_e2e.py reads them): each line the time since
    the one before it, or since the alignment's start()"""

    def __init__(self, lead):
        self.on = lead and switches.get("TRACS_STAGE_TRACE") is not None
        self.start()
        if self.on:
            try:
                import psutil
                sys.stderr.write("[stage] process start -> first alignment (interpreter, imports, metadata) %.4f s\n"
                                 % (time.time() - psutil.Process().create_time()))
            except Exception:
                pass

    def start(self):
        self.t = time.perf_counter()

    def __call__(self, name):
        if self.on:
            now = time.perf_counter()
            sys.stderr.write("[stage] %s %.4f s\n" % (name, now - self.t))
            self.t = now


# option -> (the route that stays on the device until its rows, its INFO line); distance() looks the route up by name when it dispatches
DEVICE_ROUTES = {"histogram": ("_histogram_on_device", "Saving the distance histogram for %s"),
                 "mst": ("_forest_on_device", "Saving the minimum spanning forest for %s"),
                 "ancestors": ("_ancestors_on_device", "Saving the ancestor links for %s"),
                 "tree": ("_tree_on_device", "Saving the neighbour-joining tree for %s")}


def distance(args):
    check_tree_args(args)
    check_ancestors_args(args)
    check_mst_args(args)
    check_histogram_args(args)
    check_site_args(args)
    check_sample_args(args)
    check_msa_out_args(args)
    site_files = read_site_files(args)
    groups = read_groups(args.groups) if args.histogram and args.groups is not None else None
    nearest = args.nearest
    if nearest is not None and args.gpus > 1:
        raise SystemExit("tracs distance: --nearest runs on one GPU; use --gpus 1")
    from . import multigpu
    if args.gpus > 1 and not multigpu.in_worker():
        rc = multigpu.spawn("tracs_amd", _cli_of(args), args.gpus)     # before anything here has touched the GPU
        if rc:
            raise SystemExit(rc)
        return
    ctx = multigpu.init() if multigpu.in_worker() else None
    if ctx is None:
        # the HIP runtime, the context and the library's kernels come up beside the metadata and the FASTA read (csrc/capi.hip)
        try:
            _lib.load().tracs_warm_up()
        except Exception:                                        # (no library / no GPU: the first real call says so)
            pass
    lead = ctx is None or ctx[1] == 0
    logging.basicConfig(level=args.loglevel, format="%(asctime)s - %(levelname)s - %(message)s",
                        datefmt="%Y-%m-%d %H:%M:%S")
    logging.info("Loading metadata...")
    dates = _read_dates(args.metadata) if args.metadata is not None else None
    logging.info("Estimating transmission distances...")
    tree_changes, args.tree_files_made = tree_changes_on(args), False
    if lead and not tree_changes:                  # (the changes stage of the tree request: the library creates the run's files)
        with open(args.output_file, "w") as out:
            out.write("" if args.tree is not None else HISTOGRAM_HEADER if args.histogram else HEADER)      # (Newick lines: no header)
        if args.tree is not None and args.tree_edges is not None:
            with open(args.tree_edges, "w") as out:
                out.write(tree_edges_header(args))
        if args.tree is not None and args.bootstrap_trees is not None:
            open(args.bootstrap_trees, "w").close()
        if args.ancestors is not None and args.ancestors_out is not None:
            with open(args.ancestors_out, "w") as out:
                out.write(ANCESTORS_HEADER)
    stage = _Stages(lead)
    route = next((r for opt, r in DEVICE_ROUTES.items() if vars(args)[opt]), None)
    for msa in args.msa_files:
        logging.info("Calculating pairwise snp distances for %s", msa)
        msas = [msa, args.msa_db] if args.msa_db is not None else [msa]
        stage.start()
        ref = ref_of(msa)
        rule = site_rule_for(msas, args, site_files)
        ruled = dict(rule=rule) if rule is not None else {}                 # (no rule: every route is called as it always was)
        if args.msa_out is not None or args.site_table is not None:
            ruled["contigs"] = site_files[2]
        if tree_changes:
            ruled["tree_contigs"] = site_files[2]
        if route is not None:
            # one GPU, on the device until its rows: the histogram, the forest or the ancestor links of the pairs the full run would write, or the tree
            require_files(msas)
            globals()[route[0]](msas, args, groups if args.histogram else dates, ref, stage, **ruled)      # (--histogram takes no --meta)
            logging.info(route[1], msa)
            continue
        if ctx is None and nearest is None and switches.get("TRACS_DISTANCE_ARRAYS") is None:
            # one GPU: the results stay on the device until the CSV rows (with --filter: the filtered distances and the transmission
            # model they drive too)
            require_files(msas)                              # (api.pairsnp_arrays's diagnosis; the reference passes a NULL gzFile on)
            if _rows_on_device(msas, args, dates, ref, stage, **ruled):
                logging.info("Saving distances for %s", msa)
                continue
        if ctx is None:
            # each sample's K nearest (tracs_nearest), or every pair; then the array route below: -K drops rows after the selection
            info = {}
            kw = rule.api_kwargs(info) if rule is not None else {}         # (no rule: the call as it always was)
            if nearest is not None:
                res = nearest_arrays(fasta=msas, k=nearest, n_threads=args.n_cpu, dist=args.snp_threshold, filter=args.recomb_filter, **kw)
            else:
                res = pairsnp_arrays(fasta=msas, n_threads=args.n_cpu, dist=args.snp_threshold, filter=args.recomb_filter, **kw)
            if rule is not None:
                _report_arrays(rule, args, msa, info)
            _msa_outputs_fresh(msas, args, rule, site_files[2])
        else:
            res = _pairs_multi_gpu(msas, args, ctx)
        stage("pairsnp (total, incl. the copy of the result into numpy arrays)")
        if not lead:
            continue
        rows, cols, snpd, names, filt, ncomp = res
        with_dates = dates is not None and len(rows) > 0
        tdist = ek = ddiff = None
        if with_dates:
            logging.info("Inferring transmission probabilities for %s", msa)
            # with --filter the transmission model is driven by the FILTERED distance (:183-193)
            drive = filt if args.recomb_filter else snpd
            tdist, ek, ddiff = calculate_trans_prob([rows, cols, drive], sample_dates=dates, K=100,
                                                    lamb=args.clock_rate, beta=args.trans_rate, samplenames=names,
                                                    log=False, precision=args.precision)
            if not args.recomb_filter:
                filt = None                                                     # a column of "NA" (:204)
            stage("transcluster (dates -> delta, H2D, keys, gather, D2H)")
        logging.info("Saving distances for %s", msa)
        _append_rows(args.output_file, names, rows, cols, snpd, filt, ncomp, ddiff, tdist, ek,
                     args.trans_threshold if with_dates else None, ref)
        stage("CSV rows (format + write, %d rows)" % len(rows))
    if ctx is not None:
        ctx[0].barrier()
        ctx[0].destroy_process_group()


def main():
    parser = distance_parser(argparse.ArgumentParser())
    args = parser.parse_args()
    args.func(args)


if __name__ == "__main__":
    main()
