"""The one place in Python that opens, reads and frees a tracs_distance and that builds a tracs_rules (include/tracs_hip.h).

Python calls the _rules form of every FASTA entry point (tracs_pairsnp_rules, tracs_nearest_rules, tracs_distance_open_rules): a struct
with no field set is the plain call and one with only keep / max_n_samples the _sites call (rules_from_struct, csrc/capi.hip); the other
two forms stay in the C ABI.  numpy is imported where it is needed: the plain device route of `tracs distance` runs without it.
"""
import collections
import ctypes as C
import os

from . import _lib


TreeResult = collections.namedtuple("TreeResult", "joins rows changes minimum kept branches")
# tree(iterate=K): the same counters for the final tree, then the final k, the earlier tree it repeats (None: stopped at the limit),
# the cells the last mask made N and the largest mask work W
TreeIterateResult = collections.namedtuple("TreeIterateResult", TreeResult._fields + ("iterations", "same_as", "masked_cells", "mask_work"))

OPEN_STAGE = "[sum] tracs_distance_open (read FASTA, allocate, H2D + pack)"      # the [stage] line of an open (TRACS_STAGE_TRACE)


def input_paths(fasta, existing=True):
    """The FASTA paths of an entry point, encoded; existing=False leaves the existence check to a later require_files."""
    if isinstance(fasta, (str, bytes, os.PathLike)):
        raise TypeError("pairsnp(): fasta must be a list of paths")
    paths = [os.fsencode(p) for p in fasta]
    if len(paths) < 1 or len(paths) > 2:
        raise RuntimeError("Invalid number of fasta files!")      # src/pairsnp.hpp:340-343
    return require_files(paths) if existing else paths


def require_files(paths):
    for p in paths:
        if not os.path.exists(p):
            # the reference passes a NULL gzFile on (src/pairsnp.hpp:75-76); we diagnose instead
            raise FileNotFoundError(os.fsdecode(p))
    return paths


def rules_struct(sites=None, max_sample_n_share=None, max_n_share=None, min_sites=None):
    """The site rule (tracs_amd.sites.Sites or None), the sample / pair rules and the N share of the FASTA entry points (DESIGN.md 3.12,
    3.13) -> (_lib.Rules, array to keep alive for the call).  Nothing given: the struct with no field set."""
    for name, share in (("max_sample_n_share", max_sample_n_share), ("max_n_share", max_n_share)):
        if share is not None and not (0.0 <= float(share) <= 1.0):
            raise ValueError("%s must be in [0, 1], got %r" % (name, share))
    if min_sites is not None and not (1 <= int(min_sites) <= 0xFFFFFFFF):
        raise ValueError("min_sites must be in [1, 2^32 - 1], got %r" % (min_sites,))
    if sites is not None and sites.max_n_samples is not None:
        if max_sample_n_share is not None:
            raise ValueError("Sites(max_n_samples=...) cannot be combined with max_sample_n_share: the N rule counts over the samples "
                             "that survive the sample rule, whose number is only known on the device; give max_n_share")
        if max_n_share is not None:
            raise ValueError("Sites(max_n_samples=...) and max_n_share are two forms of one rule; give one")
    words, keep_len, max_n = (None, 0, 0xFFFFFFFF) if sites is None else sites.c_args()
    r = _lib.Rules(words.ctypes.data_as(C.POINTER(C.c_uint64)) if words is not None else None, keep_len,
                   -1.0 if max_n_share is None else float(max_n_share), -1.0 if max_sample_n_share is None else float(max_sample_n_share),
                   0 if min_sites is None else int(min_sites), max_n)
    return r, words


def _names(count, name, h):
    return [name(h, i).decode("utf-8", "replace") for i in range(count(h))]


def source_records(L, kind, h):
    """What the sample rule saw (tracs_<kind>_source_*): the names of the records read, their N counts among the "rule_sites"
    file-kept columns, and which stayed -- under the keys of the array entry points' `info`"""
    import numpy as np
    get = lambda name: getattr(L, "tracs_%s_%s" % (kind, name))                     # noqa: E731
    n = get("source_nseq")(h)
    return {"source_names": _names(get("source_nseq"), get("source_name"), h),
            "n_counts": np.array([get("source_n_count")(h, i) for i in range(n)], np.uint32),
            "kept": np.array([get("source_kept")(h, i) != 0 for i in range(n)], bool),
            "rule_sites": int(get("rule_sites")(h))}


class DistanceHandle:
    """One opened tracs_distance: `with DistanceHandle(fasta, sites=..) as h`.  Freed on every way out of the block, also when a step
    between the open and the first use raises; close() may be called again."""

    def __init__(self, fasta, sites=None, max_sample_n_share=None, max_n_share=None, min_sites=None):
        paths = input_paths(fasta)
        self.h = None
        self.L = _lib.require_gpu()
        rules, alive = rules_struct(sites, max_sample_n_share, max_n_share, min_sites)      # (alive: referenced until the call returns)
        h = C.c_void_p()
        _lib.check(self.L.tracs_distance_open_rules((C.c_char_p * len(paths))(*paths), len(paths), C.byref(rules), C.byref(h)))
        self.h = h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        h, self.h = self.h, None
        if h is not None:
            self.L.tracs_distance_free(h)

    @property
    def names(self):
        return _names(self.L.tracs_distance_nseq, self.L.tracs_distance_name, self.h)

    @property
    def n(self):
        return self.L.tracs_distance_nseq(self.h)

    @property
    def length(self):
        """the columns compared (the kept ones)"""
        return self.L.tracs_distance_len(self.h)

    @property
    def source_len(self):
        """the columns of the files read"""
        return self.L.tracs_distance_source_len(self.h)

    def kept_words(self):
        """the kept columns as a bitmap over the columns read (uint64 words)"""
        import numpy as np
        kept = np.zeros((self.source_len + 63) // 64, np.uint64)
        _lib.check(self.L.tracs_distance_kept_sites(self.h, kept.ctypes.data_as(C.POINTER(C.c_uint64))))
        return kept

    def kept_positions(self):
        """the kept columns as indices into the columns read"""
        import numpy as np
        from .sites import bitmap_to_bool
        return np.flatnonzero(bitmap_to_bool(self.kept_words(), self.source_len))

    def source(self):
        return source_records(self.L, "distance", self.h)

    def tree(self, path, ref, per_site=False, edges_path=None, bootstrap=0, seed=1, replicate_trees=None, support="split",
             changes_path=None, sites_path=None, max_entries=None, contigs=None, n_threads=0, create=True, tree_filter=False,
             filtered_path=None, iterate=None, iterations_path=None, method="nj"):
        """The neighbour-joining tree of the handle's samples, or with method="bionj" their BIONJ tree (every tree of the
        call, replicates and rebuilds included; it travels as bit 1 of the request's kind): the keywords as one tracs_tree_request (include/tracs_hip.h describes every
        field) -> TreeResult, 0 where nothing was asked for.  One Newick line is appended to `path`, the edge rows to
        edges_path.  bootstrap = B > 0: B replicates under `seed`, support "split" or "transfer", each replicate's line to replicate_trees.
        changes_path / sites_path / tree_filter (no bootstrap): every site placed on the tree, at most max_entries (default 10^8) changes,
        contigs [(name, length)] or None; create: the library creates the files with their headers (False: it appends to them).
        iterate = K in [1, 100] (with tree_filter; tracs_distance_tree_iterate): the dropped changes are masked below
        their branches, the tree rebuilt, until its splits repeat or K trees were rebuilt; every file is then the final tree's, and
        iterations_path gets a row per tree -> TreeIterateResult."""
        if iterate is None:
            if iterations_path is not None:
                raise ValueError("tree(): iterations_path needs iterate")
        elif not tree_filter:
            raise ValueError("tree(): iterate needs tree_filter")
        elif bootstrap:
            raise ValueError("tree(): iterate takes no bootstrap")
        elif not 1 <= int(iterate) <= 100:
            raise ValueError("tree(): iterate must be in [1, 100]")
        if method not in ("nj", "bionj"):
            raise ValueError("tree(): method is 'nj' or 'bionj'")
        if support not in ("split", "transfer"):
            raise ValueError("tree(): support is 'split' or 'transfer'")
        if filtered_path is not None and not tree_filter:
            raise ValueError("tree(): filtered_path needs tree_filter")
        if tree_filter and edges_path is None and changes_path is None and filtered_path is None:
            raise ValueError("tree(): tree_filter needs edges_path, changes_path or filtered_path")
        changes = changes_path is not None or sites_path is not None or tree_filter
        if changes:
            if bootstrap:
                raise ValueError("tree(): changes_path / sites_path / tree_filter take no bootstrap")
            if max_entries is not None and changes_path is None and not tree_filter:
                raise ValueError("tree(): max_entries bounds the rows of changes_path")
            max_entries = 100000000 if max_entries is None else int(max_entries)
            if max_entries < 1:
                raise ValueError("tree(): max_entries must be at least 1")
        elif max_entries is not None:
            raise ValueError("tree(): max_entries needs changes_path")
        elif not bootstrap:
            if replicate_trees is not None:
                raise ValueError("tree(): replicate_trees needs bootstrap > 0")
            if support != "split":
                raise ValueError("tree(): support='transfer' needs bootstrap > 0")
        elif per_site:
            raise ValueError("tree(): bootstrap replicates take the SNP distance only (per_site=False)")
        elif not (1 <= int(bootstrap) < 2 ** 32) or not (0 <= int(seed) < 2 ** 64):
            raise ValueError("tree(): bootstrap must be in [1, 2^32) and seed in [0, 2^64)")
        enc = lambda p: os.fsencode(p) if p is not None else None         # noqa: E731
        contigs = contigs if changes and contigs else []                    # (read by the change and site rows only)
        req = _lib.TreeRequest(
            kind=int(bool(per_site)) | (_lib.TREE_BIONJ if method == "bionj" else 0), path=os.fsencode(path), ref=ref.encode(), edges_path=enc(edges_path), replicates=int(bootstrap),
            seed=int(seed), transfer=int(bool(bootstrap) and support == "transfer"), replicate_trees_path=enc(replicate_trees) if bootstrap else None,
            changes=int(changes), changes_path=enc(changes_path), sites_path=enc(sites_path), filter=int(bool(tree_filter)),
            filtered_path=enc(filtered_path), contig_names=(C.c_char_p * len(contigs))(*[c[0].encode() for c in contigs]),
            contig_lengths=(C.c_uint64 * len(contigs))(*[int(c[1]) for c in contigs]), n_contigs=len(contigs),
            max_entries=max_entries or 0, n_threads=int(n_threads), create=int(bool(create)))
        res = _lib.TreeResult()
        if iterate is not None:
            it, ires = _lib.TreeIterate(int(iterate), enc(iterations_path)), _lib.TreeIterateResult()
            _lib.check(self.L.tracs_distance_tree_iterate(self.h, C.byref(req), C.byref(it), C.byref(res), C.byref(ires)))
            return TreeIterateResult(*(getattr(res, name) for name, _ in res._fields_), ires.iterations,
                                     ires.same_as if ires.same_as >= 0 else None, ires.masked_cells_last, ires.mask_work_max)
        _lib.check(self.L.tracs_distance_tree_run(self.h, C.byref(req), C.byref(res)))
        return TreeResult(*(getattr(res, name) for name, _ in res._fields_))

    def alignment(self):
        """the handle's packed alignment, borrowed: close it before the handle"""
        from . import device as dev
        return dev.Alignment.borrowed(self.L, self.L.tracs_distance_alignment(self.h))


def run_arrays(entry, paths, k, n_threads, dist, filter, sites, info, max_sample_n_share, max_n_share, min_sites):
    """tracs_pairsnp_rules (k None) or tracs_nearest_rules on checked input_paths -> (library, result handle); info (a dict or None)
    <- "seqlen", and with one of the three rules what the sample rule saw"""
    L = _lib.require_gpu()
    rules, alive = rules_struct(sites, max_sample_n_share, max_n_share, min_sites)          # (alive: referenced until the call returns)
    h = C.c_void_p()
    head = (int(n_threads),) if k is None else (int(n_threads), k)
    _lib.check(getattr(L, entry)((C.c_char_p * len(paths))(*paths), len(paths), *head, int(dist), int(bool(filter)), C.byref(rules), C.byref(h)))
    if info is not None:
        if not (max_sample_n_share is None and max_n_share is None and min_sites is None):
            info.update(source_records(L, "pairsnp", h))
        info["seqlen"] = int(L.tracs_pairsnp_seqlen(h))
    return L, h
