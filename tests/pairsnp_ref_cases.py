"""tests/golden/pairsnp_ref_golden.npz -- what the reference's own src/pairsnp.hpp returned (oracle/_ref/_tracs_ref_pairsnp, built over
oracle/boost_standin; generator: tests/golden/make_golden.py pairsnp-ref) -- read back, and its inputs written out as FASTA files.

TEST INFRASTRUCTURE ONLY, shared by the generator, tests/test_pairsnp_ref.py and tests/test_gpu_pairsnp_ref.py.  The fixture is
self-contained: it holds the alignments themselves, never a generator seed.

Layout: "meta" is a JSON text -- {"cases": [case, ..], "filter_cases": [case, ..], "hp": {...}, "measured": {...}} -- and the arrays
are "aln/<key>" (uint8 [n, L] ASCII), "<case name>/rows|cols|d|nn|filt" (int64, the reference's five columns; filt is all zero
where filter is false), "hp/ref" (int64 [cases, 3]: ref_filter_recomb_positions of the boundary sites and the two probes of every
case of filter_hp_golden.json), "cdf/cells" (int64 [m, 4]: L, d, n, k) and "cdf/value" (float64 [m]: ref_cached_binomial_cdf(n, d / L, k)).
A case: {"name", "aln", "n0" (None: one file; else the first n0 samples are file one), "dist", "filter", "width" (0: one line per
record), "crlf", "gz"}."""
import gzip
import io
import json
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "pairsnp_ref_golden.npz")
INT_MAX = 2147483647
COLUMNS = ("rows", "cols", "d", "nn", "filt")
_CACHE = {}


def load():
    """-> (meta dict, {array name: array}), read once"""
    if "fx" not in _CACHE:
        with np.load(FIXTURE) as z:
            arrays = {k: z[k] for k in z.files if k != "meta"}
            meta = json.loads(z["meta"].tobytes().decode())
        for a in arrays.values():
            a.setflags(write=False)
        _CACHE["fx"] = (meta, arrays)
    return _CACHE["fx"]


def save(path, meta, arrays):
    """a zip of .npy members with a fixed time stamp and order: the same data gives the same bytes"""
    members = [("meta", np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8))] + sorted(arrays.items())
    with zipfile.ZipFile(path, "w") as zf:
        for name, a in members:
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(a), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, b.getvalue(), compresslevel=9)


def names_of(n):
    return ["s%d" % i for i in range(n)]


def write_fastas(case, seqs, folder):
    """the case's one or two FASTA files as the reference was given them -> [paths]"""
    n = seqs.shape[0]
    names = names_of(n)
    parts = [(0, n)] if case["n0"] is None else [(0, case["n0"]), (case["n0"], n)]
    eol = b"\r\n" if case["crlf"] else b"\n"
    paths = []
    for f, (a, b) in enumerate(parts):
        text = io.BytesIO()
        for s in range(a, b):
            text.write(b">" + names[s].encode() + eol)
            row = seqs[s].tobytes()
            w = case["width"] or max(len(row), 1)
            for o in range(0, max(len(row), 1), w):
                text.write(row[o:o + w] + eol)
        p = os.path.join(folder, "%s_%d.fa%s" % (case["name"].replace("/", "_"), f, ".gz" if case["gz"] else ""))
        if case["gz"]:
            with open(p, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as fh:
                fh.write(text.getvalue())
        else:
            with open(p, "wb") as fh:
                fh.write(text.getvalue())
        paths.append(p)
    return paths


def expected(arrays, case):
    """-> rows, cols, d, nn, filt (int64) of one case"""
    return tuple(arrays["%s/%s" % (case["name"], c)] for c in COLUMNS)


def hp_lists(H, hp_cases):
    """the position lists of filter_hp_golden.json, in the order of "hp/ref": per case the boundary sites, the probe at wh, the probe
    at wh + 1 -> [(L, d, sites)]"""
    out = []
    for c in hp_cases:
        L, d = c["L"], c["d"]
        shape = c["probe"][0]
        out.append((L, d, np.asarray(H.boundary_positions(L, d, c["row"]), np.int64)))
        out.append((L, d, np.asarray(H.probe_positions(L, d, shape, c["wh"]), np.int64)))
        out.append((L, d, np.asarray(H.probe_positions(L, d, shape, c["wh"] + 1), np.int64)))
    return out
