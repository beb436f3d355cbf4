"""tracs_amd/handle.py on a stub library that counts the open and free calls (no GPU, no libtracs_hip.so): a DistanceHandle is freed
exactly once however its block ends, the keep bitmap is alive while the library reads it, and the path checks keep their order."""
import argparse
import ctypes as C
import gc
import weakref

import numpy as np
import pytest


class StubLibrary:
    """tracs_distance_open_rules / _free counted; every other function answers 0"""

    def __init__(self, rc=0):
        self.rc, self.opened, self.freed, self.at_open = rc, 0, [], None

    def tracs_distance_open_rules(self, paths, n, rules, out):
        self.opened += 1
        if self.at_open is not None:
            self.at_open(rules._obj)
        if self.rc == 0:
            out._obj.value = 0x7ACE
        return self.rc

    def tracs_distance_free(self, h):
        self.freed.append(h.value)

    def tracs_last_error(self):
        return b"the stub refuses"

    def __getattr__(self, name):
        if not name.startswith("tracs_"):
            raise AttributeError(name)
        return lambda *a: 0


class Boom(Exception):
    pass


@pytest.fixture
def stub(monkeypatch, tmp_path):
    from tracs_amd import _lib
    lib = StubLibrary()
    monkeypatch.setattr(_lib, "require_gpu", lambda: lib)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    fa = tmp_path / "a.fa"
    fa.write_text(">s0\nACGT\n>s1\nACGA\n")
    lib.fasta = str(fa)
    return lib


def test_freed_once_on_a_normal_exit_and_close_is_idempotent(stub):
    from tracs_amd.handle import DistanceHandle
    with DistanceHandle([stub.fasta]) as h:
        assert (stub.opened, stub.freed) == (1, []) and h.h.value == 0x7ACE
    assert stub.freed == [0x7ACE]
    h.close()
    h.close()
    assert (stub.opened, stub.freed) == (1, [0x7ACE])


def test_freed_once_when_the_body_raises(stub):
    from tracs_amd.handle import DistanceHandle
    with pytest.raises(Boom):
        with DistanceHandle([stub.fasta]):
            raise Boom()
    assert (stub.opened, stub.freed) == (1, [0x7ACE])


def test_freed_once_when_the_report_raises_between_open_and_first_use(stub, monkeypatch):
    import tracs_amd.distance as di
    args = di.distance_parser(argparse.ArgumentParser()).parse_args(["--msa", stub.fasta, "-o", "o.csv", "--min-sites", "5"])
    rule = di.site_rule_for([stub.fasta], args, di.read_site_files(args))
    assert rule is not None

    def report(*a, **k):
        assert stub.opened == len(stub.freed) + 1                  # (open, not yet freed)
        raise Boom()
    monkeypatch.setattr(rule, "report", report)
    with pytest.raises(Boom):
        with di._open([stub.fasta], rule, args):
            pytest.fail("the body ran although the report raised")
    assert (stub.opened, stub.freed) == (1, [0x7ACE])
    with pytest.raises(Boom):                                       # ... and through the routes' own block
        with di._opened([stub.fasta], args, lambda name: None, rule):
            pytest.fail("the body ran although the report raised")
    assert (stub.opened, stub.freed) == (2, [0x7ACE, 0x7ACE])


def test_nothing_to_free_when_the_open_fails(stub):
    from tracs_amd.handle import DistanceHandle
    stub.rc = -1
    with pytest.raises(RuntimeError, match="the stub refuses"):
        DistanceHandle([stub.fasta])
    assert (stub.opened, stub.freed) == (1, [])


def test_the_keep_bitmap_is_alive_while_the_library_reads_it(stub, monkeypatch):
    from tracs_amd import handle
    from tracs_amd.sites import Sites, bool_to_bitmap
    keep = np.ones(130, bool)
    keep[60:70] = False
    made, seen = [], []
    real = handle.rules_struct

    def recording(*a, **k):
        r, words = real(*a, **k)
        made.append(weakref.ref(words))
        return r, words
    monkeypatch.setattr(handle, "rules_struct", recording)

    def at_open(rules):
        gc.collect()
        words = made[-1]()
        assert words is not None, "the bitmap was released before the call"
        assert C.cast(rules.keep, C.c_void_p).value == words.ctypes.data and rules.keep_len == 130
        seen.append([rules.keep[i] for i in range(3)])
    stub.at_open = at_open
    with handle.DistanceHandle([stub.fasta], sites=Sites(keep, 7), min_sites=3):
        pass
    assert seen == [bool_to_bitmap(keep).tolist()] and stub.freed == [0x7ACE]


def test_the_path_checks_and_their_order(stub, tmp_path):
    from tracs_amd.handle import DistanceHandle, input_paths
    with pytest.raises(TypeError, match=r"pairsnp\(\): fasta must be a list of paths"):
        input_paths(stub.fasta)
    for bad in ([], [stub.fasta] * 3, ["nowhere.fa"] * 3):                  # the count comes before the existence check
        with pytest.raises(RuntimeError, match="Invalid number of fasta files!"):
            input_paths(bad)
    missing = str(tmp_path / "missing.fa")
    with pytest.raises(FileNotFoundError) as e:
        input_paths([stub.fasta, missing])
    assert str(e.value) == missing
    assert input_paths([stub.fasta, missing], existing=False) == [stub.fasta.encode(), missing.encode()]
    with pytest.raises(FileNotFoundError):                                  # before the library is asked for anything
        DistanceHandle([missing])
    assert stub.opened == 0
