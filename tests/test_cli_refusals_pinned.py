"""Every refusal `tracs distance` and `tracs pair-sites` make before anything touches the GPU, word for word as the commit before
the host layer moved onto tracs_amd/handle.py made it (tests/golden/cli_refusals_golden.json, written from a checkout of that commit
by tests/golden/make_cli_refusals_golden.py).  The entries that break two rules at once pin the order of the checks."""
import json
import os

import pytest

import cli_refusal_cases as T

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_refusals_golden.json")))


def test_the_golden_holds_the_cases():
    assert [(g["command"], g["argv"]) for g in GOLDEN] == [(c, a) for c, a, _ in T.CASES]
    assert sum("before" in covers for _, _, covers in T.CASES) >= 8
    assert all(g["message"].startswith("tracs %s" % g["command"]) for g in GOLDEN)


@pytest.mark.parametrize("entry", GOLDEN, ids=["%s %s" % (g["command"], " ".join(g["argv"])) for g in GOLDEN])
def test_refusal_text_is_the_parents(tmp_path, monkeypatch, entry):
    T.write_files(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    assert T.refusal(entry["command"], entry["argv"], monkeypatch.setattr) == entry["message"]
    assert sorted(os.listdir(str(tmp_path))) == sorted(T.FILES)             # no output file, nothing else left behind
