"""Writes tests/golden/panel_walk_golden.json: sha256 and row count of every CSV that tests/test_gpu_panel_walk.py compares, as a
given build of libtracs_hip.so writes them at its default panel height.  The file in the repository comes from a build of the commit
BEFORE the host entry points shared one panel walk, so the test pins the refactored code to the bytes of the code it replaced.
The mst_* and ancestors_* entries come from a build of commit 27c4601 (before forest.hip and ancestors.hip shared csrc/pair_select.h);
that build wrote the eight older entries as they stood, so one run of this script at that commit gives the whole file.
Needs a GPU.  Inputs, routes and options are the test's own (imported from it); nothing here is an expected value.

usage: python tests/golden/make_panel_walk_golden.py DIRECTORY_WITH_libtracs_hip.so [OUT.json]"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    from tracs_amd import _lib
    _lib.LIB_PATH = os.path.join(os.path.abspath(argv[1]), "libtracs_hip.so")      # before anything loads the library
    import test_gpu_panel_walk as T
    with tempfile.TemporaryDirectory() as td:
        csv, _ = T.run_routes(T.make_inputs(td), td, None)
    out = argv[2] if len(argv) > 2 else T.GOLDEN
    with open(out, "w") as fh:
        json.dump({name: T.digest(data) for name, data in sorted(csv.items())}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%s: %d files, library %s" % (out, len(csv), _lib.LIB_PATH))


if __name__ == "__main__":
    main(sys.argv)
