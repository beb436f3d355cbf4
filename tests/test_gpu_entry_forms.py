"""The three forms of each FASTA entry point of libtracs_hip.so, called directly through ctypes: the plain one, `_sites` and `_rules`
(include/tracs_hip.h).  Python itself only calls the `_rules` form (tracs_amd/handle.py); the other two stay in the C ABI and are
held here to the same results -- without a rule all forms are one call, with a site rule `_sites(keep, L, m)` is
`_rules{keep, L, -1, -1, 0, m}`, and both are the oracle on the alignment with the dropped columns deleted.

12 samples x 300 columns: the keep bitmap has a run dropped across the seam of its first two 64-column words and part of its ragged
last word (300 = 4 * 64 + 44) dropped, so a wrong keep_len, a bitmap that is gone by the time the library reads it, or a wrong first-
file count (the two-file run, cut 5 + 7) shows."""
import ctypes as C
import os

import numpy as np
import pytest

from site_rules_common import is_n_table

pytestmark = pytest.mark.gpu
N, L, N0, K = 12, 300, 5, 3
NO_RULE = 0xFFFFFFFF
U64P = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def data(tmp_path_factory, oracle, hiplib):
    from tracs_amd import synth
    from tracs_amd.sites import bool_to_bitmap
    td = str(tmp_path_factory.mktemp("entry_forms"))
    seqs = synth.alignment(N, L, seed=2024, n_lineages=3, mu_lineage=5e-2, mu_sample=2e-2, p_n=0.06, p_partial=0.02)
    names = ["e%02d" % i for i in range(N)]
    files = {None: [os.path.join(td, "all.fa")], N0: [os.path.join(td, "query.fa"), os.path.join(td, "db.fa")]}
    synth.write_fasta(files[None][0], seqs, names=names, width=70)
    synth.write_fasta(files[N0][0], seqs[:N0], names=names[:N0])
    synth.write_fasta(files[N0][1], seqs[N0:], names=names[N0:])
    keep = np.ones(L, bool)
    keep[60:71] = False                                 # across the seam of words 0 and 1
    keep[270:281] = False                               # inside the ragged last word (columns 256 .. 299)
    keep[299] = False                                   # ... and its last column
    n_count = is_n_table(hiplib)[seqs].sum(axis=0)
    max_n = int(n_count[keep].max()) - 1                # from the data: the file-kept columns with the most N go too
    kept = keep & (n_count <= max_n)
    assert max_n >= 0 and 0 < kept.sum() < keep.sum() < L
    d = oracle.pairsnp_arrays(seqs)[2]
    dist = int(np.sort(d)[len(d) // 2])                 # the median distance: some pairs pass, not all
    out = dict(td=td, seqs=seqs, names=names, files=files, keep=keep, words=bool_to_bitmap(keep), max_n=max_n, kept=kept, dist=dist)
    for n0 in (None, N0):
        for cols in (slice(None), kept):
            dd = oracle.pairsnp_arrays(seqs[:, cols], n0=n0)[2]
            assert 0 < (dd <= dist).sum() < len(dd), (n0, "-D does not cut")
    return out


def _paths(paths):
    return (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths]), len(paths)


def _rules(keep=None, keep_len=0, max_n=NO_RULE):
    from tracs_amd import _lib
    return _lib.Rules(keep, keep_len, -1.0, -1.0, 0, max_n)


def _arrays(lib, rc, h):
    """the five arrays and the names of a tracs_pairsnp_result, copied (the result is freed with the views)"""
    from tracs_amd import _lib, api
    _lib.check(rc)
    r, c, d, names, f, nn = api._result_arrays(lib, h)
    return [np.array(x, np.uint64) for x in (r, c, d, nn, f)], names, int(lib.tracs_pairsnp_seqlen(h))


def _array_forms(lib, paths, k, dist, rule):
    """{form: (arrays, names, seqlen)} of tracs_pairsnp* (k None) or tracs_nearest* with filter on.  rule: None, or (words, L, m)"""
    arr, n = _paths(paths)
    head = (arr, n, 1) if k is None else (arr, n, 1, k)
    stem = "tracs_pairsnp" if k is None else "tracs_nearest"
    got = {}

    def call(form, fn, *tail):
        h = C.c_void_p()
        got[form] = _arrays(lib, getattr(lib, fn)(*head, dist, 1, *tail, C.byref(h)), h)
    if rule is None:
        call("plain", stem)
        call("sites", stem + "_sites", None, 0, NO_RULE)
        call("rules NULL", stem + "_rules", None)
        call("rules unset", stem + "_rules", C.byref(_rules()))
    else:
        words, length, m = rule
        kp = words.ctypes.data_as(U64P)
        call("sites", stem + "_sites", kp, length, m)
        call("rules", stem + "_rules", C.byref(_rules(kp, length, m)))
    return got


def _handle_forms(lib, paths, dist, rule, td, tag):
    """{form: (CSV bytes of tracs_distance_run, names, length, source_len, kept bitmap)} of tracs_distance_open*"""
    from tracs_amd import _lib
    arr, n = _paths(paths)
    got = {}

    def call(form, fn, *tail):
        h = C.c_void_p()
        _lib.check(getattr(lib, fn)(arr, n, *tail, C.byref(h)))
        try:
            out = os.path.join(td, "%s_%s.csv" % (tag, form.replace(" ", "_")))
            with open(out, "w") as fh:
                fh.write("header\n")
            written, pairs = C.c_uint64(0), C.c_uint64(0)
            _lib.check(lib.tracs_distance_run(h, dist, None, 1.0, 1.0, 0.01, -1.0, os.fsencode(out), b"ref", 1, C.byref(written), C.byref(pairs)))
            names = [lib.tracs_distance_name(h, i).decode() for i in range(lib.tracs_distance_nseq(h))]
            source_len = lib.tracs_distance_source_len(h)
            kept = np.zeros((source_len + 63) // 64, np.uint64)
            _lib.check(lib.tracs_distance_kept_sites(h, kept.ctypes.data_as(U64P)))
            with open(out, "rb") as fh:
                got[form] = (fh.read(), names, int(lib.tracs_distance_len(h)), int(source_len), kept.tolist(), int(written.value))
        finally:
            lib.tracs_distance_free(h)
    if rule is None:
        call("plain", "tracs_distance_open")
        call("sites", "tracs_distance_open_sites", None, 0, NO_RULE)
        call("rules NULL", "tracs_distance_open_rules", None)
        call("rules unset", "tracs_distance_open_rules", C.byref(_rules()))
    else:
        words, length, m = rule
        kp = words.ctypes.data_as(U64P)
        call("sites", "tracs_distance_open_sites", kp, length, m)
        call("rules", "tracs_distance_open_rules", C.byref(_rules(kp, length, m)))
    return got


def _all_equal(got, what):
    forms = list(got)
    first = got[forms[0]]
    for form in forms[1:]:
        for k, (a, b) in enumerate(zip(first, got[form])):
            if isinstance(a, list) and a and isinstance(a[0], np.ndarray):
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), (what, forms[0], form, k)
            else:
                assert a == b, (what, forms[0], form, k)
    return first


def _expected_pairs(oracle, seqs, n0, dist):
    r, c, d, nn = oracle.pairsnp_arrays(seqs, n0=n0, dist=dist)
    return [r, c, d, nn, oracle.filter_recomb_pairs(seqs, r, c)]


RULES = ["no rule", "site rule"]


def _case(data, ruled):
    if ruled == "no rule":
        return None, data["seqs"]
    return (data["words"], L, data["max_n"]), data["seqs"][:, data["kept"]]


@pytest.mark.parametrize("n0", [None, N0], ids=["one file", "two files"])
@pytest.mark.parametrize("ruled", RULES)
def test_pairsnp_forms(hiplib, oracle, data, n0, ruled):
    rule, seqs = _case(data, ruled)
    arrays, names, seqlen = _all_equal(_array_forms(hiplib, data["files"][n0], None, data["dist"], rule), "pairsnp")
    assert names == data["names"] and seqlen == seqs.shape[1]
    for g, e in zip(arrays, _expected_pairs(oracle, seqs, n0, data["dist"])):
        assert np.array_equal(g, e)
    assert len(arrays[0]) > 0


@pytest.mark.parametrize("n0", [None, N0], ids=["one file", "two files"])
@pytest.mark.parametrize("ruled", RULES)
def test_nearest_forms(hiplib, oracle, data, n0, ruled):
    from test_gpu_nearest import expected
    rule, seqs = _case(data, ruled)
    arrays, names, seqlen = _all_equal(_array_forms(hiplib, data["files"][n0], K, data["dist"], rule), "nearest")
    assert names == data["names"] and seqlen == seqs.shape[1]
    exp = expected(oracle, seqs, K, n0=n0, dist=data["dist"])
    for g, e in zip(arrays[:4], exp):
        assert np.array_equal(g, e)
    # the filtered distance of an emitted pair is that of the pair, whichever of its samples lists it
    lo, hi = np.minimum(exp[0], exp[1]), np.maximum(exp[0], exp[1])
    assert np.array_equal(arrays[4], oracle.filter_recomb_pairs(seqs, lo, hi))
    assert len(arrays[0]) > 0


@pytest.mark.parametrize("n0", [None, N0], ids=["one file", "two files"])
@pytest.mark.parametrize("ruled", RULES)
def test_distance_open_forms(hiplib, oracle, data, n0, ruled):
    from tracs_amd.sites import bool_to_bitmap
    rule, seqs = _case(data, ruled)
    tag = "%s_%s" % ("one" if n0 is None else "two", ruled.split()[0])
    csv, names, length, source_len, kept, written = _all_equal(_handle_forms(hiplib, data["files"][n0], data["dist"], rule, data["td"], tag),
                                                               "distance_open")
    assert names == data["names"] and (length, source_len) == (seqs.shape[1], L)
    assert kept == bool_to_bitmap(data["kept"] if rule is not None else np.ones(L, bool)).tolist()
    r, c, d, nn, f = _expected_pairs(oracle, seqs, n0, data["dist"])
    rows = [ln.split(",") for ln in csv.decode().split("\n")[1:-1]]
    assert written == len(rows) == len(r) > 0
    exp = [[names[int(i)], names[int(j)], str(int(a)), str(int(b)), str(int(m)), "ref"] for i, j, a, m, b in zip(r, c, d, nn, f)]
    assert [[x[0], x[1], x[3], x[6], x[7], x[8]] for x in rows] == exp      # (no dates: the other three columns hold no number)
