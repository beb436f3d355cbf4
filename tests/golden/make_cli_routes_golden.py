"""Writes tests/golden/cli_routes_golden.json: what every route of tests/cli_routes_common.py wrote (sha256 and line count per file)
and logged (the INFO messages, the [stage] names) and the keys the API left in `info`, as a given checkout's tracs_amd package does it
on the GPU.  The file in the repository comes from a checkout of the commit BEFORE the host layer moved onto tracs_amd/handle.py,
running on this tree's build of libtracs_hip.so (csrc/ is the same in both), so tests/test_gpu_cli_routes_pinned.py pins the
refactored Python layer to the bytes and the log of the code it replaced.  Needs a GPU.  Inputs, routes and options are the test's
own (imported); nothing here is an expected value.

usage: python tests/golden/make_cli_routes_golden.py PARENT_TREE [OUT.json]"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    parent = os.path.abspath(argv[1])
    sys.path[:0] = [parent, os.path.join(ROOT, "tests"), ROOT]               # tracs_amd: the parent's; the routes and the oracle: this tree's
    import tracs_amd
    from tracs_amd import _lib, api
    assert os.path.dirname(os.path.dirname(os.path.abspath(tracs_amd.__file__))) == parent, tracs_amd.__file__
    if not os.path.exists(_lib.LIB_PATH):
        _lib.LIB_PATH = os.path.join(ROOT, "tracs_amd", "lib", "libtracs_hip.so")      # before anything loads the library
    import cli_routes_common as T
    from site_rules_common import is_n_table
    out = os.path.abspath(argv[2] if len(argv) > 2 else os.path.join(HERE, "cli_routes_golden.json"))
    with tempfile.TemporaryDirectory() as td:
        inp = T.make_inputs(td)
        isn = is_n_table(_lib.load())
        m = T.min_sites_of(inp, isn)
        got = {"routes": {r[0]: T.run_route(inp, r) for r in T.routes(inp, m)}, "api_info_keys": {}}
        for name, (fn, head, kw) in T.api_calls(inp, m, T.max_n_of(inp, isn)).items():
            info = {}
            getattr(api, fn)([inp["fa"]], *head, info=info, **kw)
            got["api_info_keys"][name] = sorted(info)
    with open(out, "w") as fh:
        json.dump(got, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%s: %d routes, package %s, library %s" % (out, len(got["routes"]), os.path.dirname(tracs_amd.__file__), _lib.LIB_PATH))


if __name__ == "__main__":
    main(sys.argv)
