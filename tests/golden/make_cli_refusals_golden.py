"""Writes tests/golden/cli_refusals_golden.json: the text with which `tracs distance` and `tracs pair-sites` refuse each command line
of tests/cli_refusal_cases.py, as a given checkout's tracs_amd package words it.  The file in the repository comes from a checkout of
the commit BEFORE the host layer moved onto tracs_amd/handle.py, so tests/test_cli_refusals_pinned.py pins the refactored checks to
the texts, and to the order, of the code they replaced.  Needs no GPU and no built library: every way to one is replaced by a
function that fails.  The command lines are the test's own (imported); nothing here is an expected value.

usage: python tests/golden/make_cli_refusals_golden.py PARENT_TREE [OUT.json]"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    sys.path[:0] = [os.path.abspath(argv[1]), os.path.dirname(HERE)]      # tracs_amd: the parent's; the cases: this tree's
    import tracs_amd
    import cli_refusal_cases as T
    assert os.path.dirname(os.path.dirname(os.path.abspath(tracs_amd.__file__))) == os.path.abspath(argv[1]), tracs_amd.__file__
    out = os.path.abspath(argv[2] if len(argv) > 2 else os.path.join(HERE, "cli_refusals_golden.json"))
    got = []
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        T.write_files(td)
        for command, argv_, _ in T.CASES:
            got.append({"command": command, "argv": argv_, "message": T.refusal(command, argv_, setattr)})
            assert sorted(os.listdir(td)) == sorted(T.FILES), (argv_, os.listdir(td))
        os.chdir(HERE)
    with open(out, "w") as fh:
        json.dump(got, fh, indent=1)
        fh.write("\n")
    print("%s: %d command lines, package %s" % (out, len(got), os.path.dirname(tracs_amd.__file__)))


if __name__ == "__main__":
    main(sys.argv)
