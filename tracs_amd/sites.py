"""Site rules of `tracs distance`: which columns of an alignment feed the pair matrix.

A run with a site rule is, by definition, the run on the alignment with the dropped columns deleted from every record.  This
module is the host side: BED files -> column intervals -> the keep bitmap the library takes (include/tracs_hip.h:
tracs_alignment_select_sites), the N-share threshold, and the BED of the columns a run kept.  Nothing here touches the GPU.

Columns are the reference's contigs concatenated in file order, as `align-post` writes them (align_post.read_contigs).
"""
import gzip
import math

import numpy as np

ALIGNMENT_CONTIG = "alignment"          # the contig name write_kept_bed uses without a reference


class Sites:
    """A site rule for api.pairsnp_arrays / nearest_arrays / distance_histogram: keep = bool array over the columns of the files
    (None: every column may stay), max_n_samples = a column stays only if at most that many samples are N there (None: no rule)."""

    def __init__(self, keep=None, max_n_samples=None):
        self.keep = None if keep is None else np.ascontiguousarray(keep, dtype=bool)
        if self.keep is not None and self.keep.ndim != 1:
            raise ValueError("Sites: keep must be one bool per column")
        if max_n_samples is not None and (int(max_n_samples) < 0 or int(max_n_samples) >= 0xFFFFFFFF):
            raise ValueError("Sites: max_n_samples must be in [0, 2^32 - 2]")
        self.max_n_samples = None if max_n_samples is None else int(max_n_samples)

    def active(self):
        return self.keep is not None or self.max_n_samples is not None

    def c_args(self):
        """(words or None, keep_len, max_n_samples as the library takes it): keep the first alive for the call"""
        words = None if self.keep is None else bool_to_bitmap(self.keep)
        return words, (0 if self.keep is None else len(self.keep)), (0xFFFFFFFF if self.max_n_samples is None else self.max_n_samples)


def bool_to_bitmap(keep):
    """bool[L] -> uint64 words, bit s of word s // 64 = keep[s]"""
    keep = np.ascontiguousarray(keep, dtype=bool)
    pad = (-len(keep)) % 64
    bits = np.concatenate([keep, np.zeros(pad, bool)]) if pad else keep
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


def bitmap_to_bool(words, L):
    """uint64 words -> bool[L]"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    return np.unpackbits(words.astype("<u8").view(np.uint8), bitorder="little")[:L].astype(bool)


def _merge(intervals):
    out = []
    for s, e in sorted(intervals):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return [(s, e) for s, e in out]


def contig_offsets(contigs):
    """{name: (offset, length)} of [(name, length)] in file order"""
    out, off = {}, 0
    for name, length in contigs:
        if name in out:
            raise ValueError("reference lists contig '%s' twice" % name)
        out[name] = (off, int(length))
        off += int(length)
    return out


def read_bed(path, contigs=None):
    """BED (0-based, half-open, whitespace-separated; '#', 'track', 'browser' and blank lines skipped) -> merged, sorted
    [(start, end)] in alignment columns.  contigs: [(name, length)] of the reference (align_post.read_contigs): a line's
    coordinates are shifted by its contig's offset; an unknown contig or an end beyond its contig is an error.  Without contigs
    every line must name the same contig and the coordinates are alignment columns.  start >= end is an error."""
    offsets = contig_offsets(contigs) if contigs is not None else None
    opener = gzip.open if _is_gzip(path) else open
    got, only = [], None
    with opener(path, "rt") as fh:
        for ln, line in enumerate(fh, 1):
            text = line.strip()
            if not text or text.startswith("#") or text.startswith("track") or text.startswith("browser"):
                continue
            f = text.split()
            if len(f) < 3:
                raise ValueError("%s line %d: expected contig, start, end" % (path, ln))
            try:
                start, end = int(f[1]), int(f[2])
            except ValueError:
                raise ValueError("%s line %d: start and end must be integers" % (path, ln))
            if start < 0 or start >= end:
                raise ValueError("%s line %d: empty or reversed interval [%d, %d)" % (path, ln, start, end))
            if offsets is None:
                if only is None:
                    only = f[0]
                elif f[0] != only:
                    raise ValueError("%s line %d: contigs '%s' and '%s' -- a BED with several contigs needs --mask-reference"
                                     % (path, ln, only, f[0]))
                got.append((start, end))
            else:
                if f[0] not in offsets:
                    raise ValueError("%s line %d: contig '%s' is not in the reference" % (path, ln, f[0]))
                off, length = offsets[f[0]]
                if end > length:
                    raise ValueError("%s line %d: [%d, %d) reaches past the end of contig '%s' (%d)" % (path, ln, start, end, f[0], length))
                got.append((off + start, off + end))
    return _merge(got)


def _is_gzip(path):
    with open(path, "rb") as f:
        return f.read(2) == b"\x1f\x8b"


def _paint(L, intervals, what):
    out = np.zeros(L, bool)
    for s, e in intervals:
        if e > L:
            raise ValueError("%s interval [%d, %d) reaches past the alignment's length (%d)" % (what, s, e, L))
        out[s:e] = True
    return out


def keep_bool(L, keep=None, mask=None):
    """bool[L]: the columns that may stay -- inside `keep` (intervals; None: everywhere) and outside `mask` (intervals)"""
    L = int(L)
    out = np.ones(L, bool) if keep is None else _paint(L, keep, "--keep")
    if mask is not None:
        out &= ~_paint(L, mask, "--mask")
    return out


def keep_bitmap(L, keep=None, mask=None):
    """The keep bitmap of tracs_alignment_select_sites: uint64 words, bit s of word s // 64 = column s may stay.  keep / mask:
    [(start, end)] in alignment columns (read_bed); together: keep minus mask.  An interval past L is an error."""
    return bool_to_bitmap(keep_bool(L, keep, mask))


def max_n_samples(share, n):
    """--max-n-share F: a column is dropped when more than floor(F n) samples are N there"""
    return math.floor(share * n)


def kept_runs(kept, L):
    """[(start, end)] of the set runs of kept (bool[L], or uint64 words)"""
    kept = np.asarray(kept)
    b = bitmap_to_bool(kept, L) if kept.dtype != bool else kept[:L]
    edge = np.flatnonzero(np.diff(np.concatenate([[0], b.astype(np.int8), [0]])))
    return [(int(s), int(e)) for s, e in zip(edge[0::2], edge[1::2])]


def write_kept_bed(path, kept, L, contigs=None):
    """BED of the kept runs, readable back through read_bed / --keep.  contigs ([(name, length)]): contig coordinates, runs cut at
    contig ends; without: one contig named 'alignment', alignment columns."""
    runs = kept_runs(kept, L)
    with open(path, "w") as fh:
        if contigs is None:
            for s, e in runs:
                fh.write("%s\t%d\t%d\n" % (ALIGNMENT_CONTIG, s, e))
            return
        bounds, off = [], 0
        for name, length in contigs:
            bounds.append((name, off, off + int(length)))
            off += int(length)
        if L > off:
            raise ValueError("the alignment (%d columns) is longer than the reference's contigs (%d)" % (L, off))
        k = 0
        for s, e in runs:
            while s < e:
                while bounds[k][2] <= s:
                    k += 1
                name, b0, b1 = bounds[k]
                cut = min(e, b1)
                fh.write("%s\t%d\t%d\n" % (name, s - b0, cut - b0))
                s = cut


def first_record_length(path):
    """Length of the first record of a FASTA (plain or gzip) without reading the rest: the alignment's length"""
    opener = gzip.open if _is_gzip(path) else open
    n, seen = 0, False
    with opener(path, "rb") as fh:
        for line in fh:
            if line.startswith(b">"):
                if seen:
                    break
                seen = True
            elif seen:
                n += len(line.strip())
    return n


SITE_TABLE_HEADER = "contig,position,A,C,G,T,N,other,differs\n"


def write_site_table(path, positions, counts, differs, contigs=None):
    """--site-table: one row per kept column, in order -- contig,position,A,C,G,T,N,other,differs.  positions: the kept columns in
    the coordinates of the files read (int array); counts: [6, K] (device.Alignment.site_census's rows); differs: bool[K].
    contigs ([(name, length)]): contig coordinates as write_kept_bed gives them; without: contig 'alignment', alignment columns."""
    positions = np.asarray(positions, dtype=np.int64)
    counts = np.asarray(counts)
    differs = np.asarray(differs, dtype=bool)
    if counts.shape != (6, len(positions)) or differs.shape != (len(positions),):
        raise ValueError("write_site_table: %d positions, counts %s, differs %s" % (len(positions), counts.shape, differs.shape))
    if contigs is None:
        pieces = [(ALIGNMENT_CONTIG, 0, len(positions), 0)]
    else:
        pieces, off = [], 0
        for name, length in contigs:
            lo, hi = np.searchsorted(positions, [off, off + int(length)])
            if hi > lo:
                pieces.append((name, int(lo), int(hi), off))
            off += int(length)
        if len(positions) and positions[-1] >= off:
            raise ValueError("the alignment reaches column %d, past the reference's contigs (%d)" % (int(positions[-1]), off))
    with open(path, "w") as fh:
        fh.write(SITE_TABLE_HEADER)
        step = 1 << 16
        for name, lo, hi, off in pieces:
            for b in range(lo, hi, step):
                e = min(hi, b + step)
                cols = [positions[b:e] - off] + [counts[c, b:e] for c in range(6)] + [differs[b:e].astype(np.int64)]
                fh.write("".join("%s,%d,%d,%d,%d,%d,%d,%d,%d\n" % ((name,) + row) for row in zip(*[c.tolist() for c in cols])))
