"""The tree request of the cross-compiled library without a GPU (include/tracs_hip.h: tracs_tree_request, tracs_tree_result,
tracs_distance_tree_run): the refusals that need no handle, the ctypes mirrors of the two structs against what a C
compiler makes of the header, and the edge file's header as the library spells it against the constants of tracs_amd.distance."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_null_handle_or_request_is_refused_and_the_result_zeroed(hiplib):
    from tracs_amd import _lib
    req = _lib.TreeRequest(path=b"o.nwk", ref=b"r")
    for request in (C.byref(req), None):
        res = _lib.TreeResult(*[7] * 6)
        assert hiplib.tracs_distance_tree_run(None, request, C.byref(res)) == -1
        assert hiplib.tracs_last_error().startswith(b"tracs_distance_tree_run:")
        assert [getattr(res, name) for name, _ in res._fields_] == [0] * 6
    assert hiplib.tracs_distance_tree_run(None, C.byref(req), None) == -1          # (no result asked for: refused all the same)
    assert "tracs_distance_tree_run" in _lib.SYMBOLS


def test_the_ctypes_mirrors_have_the_layout_of_the_header(tmp_path):
    """sizeof and every offsetof, printed by a C program that includes the header, against the two ctypes.Structure classes"""
    from tracs_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    structs = (("tracs_tree_request", _lib.TreeRequest), ("tracs_tree_result", _lib.TreeResult))
    lines = ['#include <stdio.h>', '#include "tracs_hip.h"', 'int main(void)', '{']
    for cname, cls in structs:
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f, _ in cls._fields_]
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {}
    for cname, cls in structs:
        want[cname] = str(C.sizeof(cls))
        want.update({"%s.%s" % (cname, f): str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert got == want
    assert len(_lib.TreeRequest._fields_) == 19 and len(_lib.TreeResult._fields_) == 6


def test_the_library_spells_the_edge_headers_as_the_cli_does(hiplib):
    """every TREE_EDGES_*_HEADER of tracs_amd.distance is tree_edges_header's text for the columns of its route (nj.hip: the writer's own
    field order), and tree_edges_header(args) picks it"""
    import argparse

    import tracs_amd.distance as di

    def library(support=0, transfer=0, changes=0, filtered=0):
        out = C.create_string_buffer(128)
        assert hiplib.tracs_debug_tree_edges_header(support, transfer, changes, filtered, out, len(out)) == 0
        return out.value.decode()
    routes = {"TREE_EDGES_HEADER": (dict(), []),
              "TREE_EDGES_SUPPORT_HEADER": (dict(support=1), ["--bootstrap", "4"]),
              "TREE_EDGES_TRANSFER_HEADER": (dict(support=1, transfer=1), ["--bootstrap", "4", "--bootstrap-support", "transfer"]),
              "TREE_EDGES_CHANGES_HEADER": (dict(changes=1), ["--tree-sites", "s.csv"]),
              "TREE_EDGES_FILTER_HEADER": (dict(changes=1, filtered=1), ["--tree-filter"])}
    assert sorted(routes) == sorted(name for name in vars(di) if name.startswith("TREE_EDGES_") and name.endswith("HEADER"))
    parser = di.distance_parser(argparse.ArgumentParser())
    for name, (columns, options) in routes.items():
        assert library(**columns) == getattr(di, name), name
        args = parser.parse_args(["--msa", "x.fa", "-o", "o.nwk", "--tree", "nj", "--tree-edges", "e.csv"] + options)
        assert di.tree_edges_header(args) == getattr(di, name), name
    assert hiplib.tracs_debug_tree_edges_header(1, 1, 1, 1, C.create_string_buffer(8), 8) == -1          # (a buffer too small is refused)
