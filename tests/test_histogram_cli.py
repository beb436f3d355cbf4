"""`tracs distance --histogram [--groups]` on the host: parser defaults, every refusal before a GPU path is entered, the groups file
rules, the label numbering, and the new symbols of the cross-compiled library."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest


def _parser():
    from tracs_amd.distance import distance_parser
    return distance_parser(argparse.ArgumentParser())


def test_defaults_off():
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.csv"])
    assert a.histogram is False and a.groups is None
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.csv", "--histogram", "--groups", "g.csv"])
    assert a.histogram is True and a.groups == os.path.abspath("g.csv")


def _no_gpu(monkeypatch):
    import tracs_amd.distance as di
    from tracs_amd import _lib, multigpu

    def no_gpu(*a, **k):
        raise AssertionError("a GPU path was entered")
    monkeypatch.setattr(multigpu, "spawn", no_gpu)
    monkeypatch.setattr(multigpu, "init", no_gpu)
    for name in ("nearest_arrays", "pairsnp_arrays", "_rows_on_device", "_forest_on_device", "_histogram_on_device"):
        monkeypatch.setattr(di, name, no_gpu)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(_lib, "load", no_gpu)


REFUSALS = [
    (["--groups", "g.csv"], ["--groups", "--histogram"]),
    (["--histogram", "--nearest", "3"], ["--histogram", "--nearest"]),
    (["--histogram", "--mst", "snp"], ["--histogram", "--mst"]),
    (["--histogram", "--gpus", "2"], ["--histogram", "--gpus"]),
    (["--histogram", "--meta", "m.csv"], ["--histogram", "--meta"]),
    (["--histogram", "-K", "3"], ["--histogram", "-K"]),
]


@pytest.mark.parametrize("extra,words", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_refusals_before_any_gpu_path(tmp_path, monkeypatch, extra, words):
    _no_gpu(monkeypatch)
    out = tmp_path / "o.csv"
    a = _parser().parse_args(["--msa", "x.fa", "-o", str(out)] + extra)
    with pytest.raises(SystemExit) as e:
        a.func(a)
    msg = str(e.value.code)
    assert msg.startswith("tracs distance: ")
    for w in words:
        assert w in msg, (w, msg)
    assert not os.path.exists(out)


def _groups_file(tmp_path, text):
    p = tmp_path / "groups.csv"
    p.write_text(text)
    return str(p)


def test_groups_file_rules(tmp_path):
    from tracs_amd.api import group_labels
    from tracs_amd.distance import read_groups
    g = read_groups(_groups_file(tmp_path, "sample,group\ns1,A\ns2,B\ns3,\ns4,A\nnot_in_alignment,Z\ns2,B\ns6\n"))
    assert "sample" not in g                                          # header line skipped
    assert g == {"s1": "A", "s2": "B", "s3": None, "s4": "A", "not_in_alignment": "Z", "s6": None}
    lab = group_labels(["s0", "s1", "s2", "s3", "s4", "s5", "s6"], g)
    assert lab.dtype == np.int32
    # s0, s5: not listed; s3, s6: empty label; the listed name that is not in the alignment is ignored
    assert lab.tolist() == [-1, 0, 1, -1, 0, -1, -1]
    assert group_labels(["s1"], None) is None
    assert group_labels(["a", "b", "c"], {"a": 7, "b": ("x", 1), "c": 7}).tolist() == [0, 1, 0]      # any hashable label


def test_groups_conflicting_duplicate_is_an_error(tmp_path, monkeypatch):
    from tracs_amd.distance import read_groups
    path = _groups_file(tmp_path, "sample,group\ns1,A\ns2,B\ns1,C\n")
    with pytest.raises(SystemExit) as e:
        read_groups(path)
    assert "'s1'" in str(e.value.code) and "two different labels" in str(e.value.code) and "'A'" in str(e.value.code) and "'C'" in str(e.value.code)
    # and the command stops there, before the GPU
    _no_gpu(monkeypatch)
    out = tmp_path / "o.csv"
    a = _parser().parse_args(["--msa", "x.fa", "-o", str(out), "--histogram", "--groups", path])
    with pytest.raises(SystemExit) as e:
        a.func(a)
    assert "'s1'" in str(e.value.code) and not os.path.exists(out)


def test_histogram_takes_its_own_route(tmp_path, monkeypatch):
    """--histogram writes its own header and hands each --msa file to _histogram_on_device with the parsed groups and the MSA file value."""
    import tracs_amd.distance as di
    seen = []

    def refuse(*a, **k):
        raise AssertionError("--histogram must not take a pair route")
    for name in ("nearest_arrays", "pairsnp_arrays", "_rows_on_device", "_forest_on_device"):
        monkeypatch.setattr(di, name, refuse)
    monkeypatch.setattr(di, "_histogram_on_device", lambda msas, args, groups, ref, stage: seen.append((msas, groups, ref)))
    fa, fb, db = tmp_path / "ref1_combined.fasta", tmp_path / "ref2.fasta.gz", tmp_path / "db.fa"
    for p in (fa, fb, db):
        p.write_text(">a\nACGT\n>b\nACGA\n")
    out = tmp_path / "o.csv"
    gp = _groups_file(tmp_path, "sample,group\na,1\nb,1\n")
    a = _parser().parse_args(["--msa", str(fa), str(fb), "--msa-db", str(db), "-o", str(out), "--histogram", "--groups", gp, "--filter",
                              "-D", "40", "--loglevel", "ERROR"])
    a.func(a)
    assert out.read_text() == "column,distance,within,between,ungrouped,MSA file\n" == di.HISTOGRAM_HEADER
    assert seen == [([str(fa), str(db)], {"a": "1", "b": "1"}, "ref1"), ([str(fb), str(db)], {"a": "1", "b": "1"}, "ref2")]
    # without --groups: no labels at all
    seen.clear()
    a = _parser().parse_args(["--msa", str(fa), "-o", str(out), "--histogram", "--loglevel", "ERROR"])
    a.func(a)
    assert seen == [([str(fa)], None, "ref1")]


def test_read_histogram_rows(tmp_path):
    from tracs_amd.api import read_histogram_rows
    p = tmp_path / "h.csv"
    p.write_text("column,distance,within,between,ungrouped,MSA file\nsnp,0,12,0,3,ref1\nsnp,4,40,2,18446744073709551615,ref1\n"
                 "filter,0,1,2,3,ref1\nsnp,9,1,1,1,ref,2\n")
    got = read_histogram_rows(str(p))
    v, w, b, u = got["snp"]["ref1"]
    assert v.dtype == np.uint32 and w.dtype == b.dtype == u.dtype == np.uint64
    assert v.tolist() == [0, 4] and w.tolist() == [12, 40] and b.tolist() == [0, 2] and u.tolist() == [3, 2 ** 64 - 1]
    assert got["filter"]["ref1"][3].tolist() == [3] and got["snp"]["ref,2"][0].tolist() == [9]


def test_library_has_the_histogram_symbols(hiplib):
    from tracs_amd import _lib
    names = ["tracs_hist_state_bytes", "tracs_hist_init", "tracs_hist_update", "tracs_hist_update_coo", "tracs_hist_emit",
             "tracs_distance_histogram", "tracs_debug_hist_routes"]
    for name in names:
        assert hasattr(hiplib, name), name
    for name in names[:-1]:
        assert name in _lib.SYMBOLS
    vp, sz = C.c_void_p, C.c_size_t
    assert hiplib.tracs_hist_state_bytes.restype is sz and hiplib.tracs_hist_state_bytes.argtypes == [sz]
    assert hiplib.tracs_hist_init.argtypes == [vp, sz, vp]
    assert hiplib.tracs_hist_update.argtypes == [vp, sz, sz, sz, sz, sz, C.c_int32, vp, vp, sz, vp]
    assert hiplib.tracs_hist_update_coo.argtypes == [vp, vp, vp, sz, vp, vp, sz, vp]
    assert hiplib.tracs_hist_emit.argtypes == [vp, sz, C.POINTER(sz), vp, vp, vp, vp, vp]
    assert len(hiplib.tracs_distance_histogram.argtypes) == 8
    # the entry points that do not touch the device: three 64-bit counts per bin and room for the emit's scratch; argument errors
    assert hiplib.tracs_hist_state_bytes(0) == 0 and hiplib.tracs_hist_state_bytes(2 ** 31 + 1) == 0
    for nb in (1, 1000, 5_000_001):
        assert hiplib.tracs_hist_state_bytes(nb) >= 24 * nb
    assert hiplib.tracs_hist_state_bytes(5_000_001) < 25 * 5_000_001
    assert hiplib.tracs_hist_init(None, 10, None) == -1 and b"tracs_hist_init" in hiplib.tracs_last_error()
    assert hiplib.tracs_hist_update(None, 4, 4, 0, 4, 0, 10, None, None, 10, None) == -1
    n = sz(0)
    assert hiplib.tracs_hist_emit(None, 10, C.byref(n), None, None, None, None, None) == -1
    assert hiplib.tracs_distance_histogram(None, 10, 0, None, b"x", b"r", None, None) == -1
    assert hiplib.tracs_abi_version() == 1


def test_kernels_are_in_the_code_object(hiplib):
    from tracs_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"hist_panel_kernel" in blob and b"hist_coo_kernel" in blob and b"hist_fill_kernel" in blob
