"""`tracs threshold` on the host: the fit on (value, count) pairs against the reference's own fit on raw lists
(tests/golden/threshold_golden.json, written by tests/golden/make_threshold_golden.py from the reference's tracs/threshold.py with the
mixture's sign corrected), the two input forms, the output file and the error messages."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XATOL = 1e-4          # SciPy's Nelder-Mead xatol: the resolution to which the reference's own answer is determined by its stopping rule


def _cases(golden_dir):
    with open(os.path.join(golden_dir, "threshold_golden.json")) as fh:
        return json.load(fh)["cases"]


def _parser():
    from tracs_amd.threshold import threshold_parser
    return threshold_parser(argparse.ArgumentParser())


def _run(argv):
    a = _parser().parse_args(argv)
    return a.func(a)


def _write_histogram(path, case, which="snp", refs=("refA",), extra=()):
    """The case as a `distance --histogram` file: within = close, between = distant, split over `refs` (their counts sum to the case's)."""
    close, distant = dict(map(tuple, case["close"])), dict(map(tuple, case["distant"]))
    with open(path, "w") as fh:
        fh.write("column,distance,within,between,ungrouped,MSA file\n")
        for k, ref in enumerate(refs):
            for v in sorted(set(close) | set(distant)):
                w, b = close.get(v, 0), distant.get(v, 0)
                share = lambda c: c // len(refs) + (1 if k < c % len(refs) else 0)      # noqa: E731
                if share(w) or share(b):
                    fh.write("%s,%d,%d,%d,%d,%s\n" % (which, v, share(w), share(b), 7, ref))
        for line in extra:
            fh.write(line + "\n")


def _write_raw(path, hist, as_float=False, seed=0):
    """The sample expanded to one row per pair, shuffled: name columns around the distance in column 1."""
    vals = np.repeat([v for v, _ in hist], [c for _, c in hist])
    np.random.default_rng(seed).shuffle(vals)
    with open(path, "w") as fh:
        fh.write("pair,distance,other\n")
        for t, v in enumerate(vals):
            fh.write("p%d,%s,x\n" % (t, ("%d.0" % v) if as_float else str(v)))


def test_golden_has_the_three_kinds_of_case(golden_dir):
    cases = {c["name"]: c for c in _cases(golden_dir)}
    assert {"simulated", "alignment", "few_close"} <= set(cases)
    assert 80 <= sum(c for _, c in cases["few_close"]["close"]) <= 120
    for c in cases.values():
        assert c["r"] < 1e4 and 0 < c["q"] < 1 and c["lambda"] > 0


@pytest.mark.parametrize("name", ["simulated", "alignment", "few_close"])
def test_fit_on_counts_equals_the_reference_fit_on_raw_lists(golden_dir, name):
    from tracs_amd import threshold as th
    case = {c["name"]: c for c in _cases(golden_dir)}[name]
    res = th.fit(dict(map(tuple, case["close"])), dict(map(tuple, case["distant"])))
    for k in ("r", "p", "q", "lambda"):
        print(name, k, "got", repr(res[k]), "reference", repr(case[k]), "difference", abs(res[k] - case[k]), "spread", case["spread"][k])
    assert res["snp_threshold"] == case["snp_threshold"]
    for k in ("r", "p", "q", "lambda"):
        assert abs(res[k] - case[k]) <= max(XATOL, 10 * case["spread"][k]), (k, res[k], case[k])
    assert res["converged"] is True
    assert res["n_close"] == sum(c for _, c in case["close"]) and res["n_distant"] == sum(c for _, c in case["distant"])
    # (values, counts) arrays are the same input as the dict
    res2 = th.fit(tuple(np.array(case["close"]).T), tuple(np.array(case["distant"]).T))
    assert res2 == res


def test_mixture_is_maximised_not_minimised(golden_dir):
    """The reference as written minimises +sum(log-likelihood) and ends at lambda ~ 0, threshold 0; the fit here
    recovers the simulated Poisson(3) component."""
    from tracs_amd import threshold as th
    case = {c["name"]: c for c in _cases(golden_dir)}["simulated"]
    res = th.fit(dict(map(tuple, case["close"])), dict(map(tuple, case["distant"])))
    assert 2.5 < res["lambda"] < 3.5 and 0.25 < res["q"] < 0.35 and res["snp_threshold"] == 18.0


@pytest.mark.parametrize("name", ["alignment", "few_close"])
def test_both_input_forms_write_the_same_file(golden_dir, tmp_path, name):
    case = {c["name"]: c for c in _cases(golden_dir)}[name]
    hist = str(tmp_path / "hist.csv")
    _write_histogram(hist, case, refs=("refA", "refB"), extra=["filter,0,5,5,5,refA"])
    _write_raw(str(tmp_path / "close.csv"), case["close"])
    _write_raw(str(tmp_path / "distant.csv"), case["distant"], as_float=True, seed=1)
    out_h, out_r = str(tmp_path / "h.csv"), str(tmp_path / "r.csv")
    res = _run(["--histogram", hist, "-o", out_h])
    _run(["--close", str(tmp_path / "close.csv"), "--distant", str(tmp_path / "distant.csv"), "--column", "1", "-o", out_r])
    assert open(out_h).read() == open(out_r).read()
    lines = open(out_h).read().split("\n")
    assert lines[0] == "parameter,value" and lines[-1] == ""
    rows = [ln.split(",") for ln in lines[1:-1]]
    assert [r[0] for r in rows] == ["r", "p", "q", "lambda", "snp_threshold", "n_close", "n_distant", "converged"]
    got = dict(rows)
    for k in ("r", "p", "q", "lambda", "snp_threshold"):
        assert got[k] == repr(res[k]) and float(got[k]) == res[k]
    assert got["snp_threshold"] == repr(case["snp_threshold"])
    assert got["n_close"] == str(sum(c for _, c in case["close"])) and got["n_distant"] == str(sum(c for _, c in case["distant"]))
    assert got["converged"] == "True"


def test_which_selects_the_column_block(golden_dir, tmp_path):
    cases = {c["name"]: c for c in _cases(golden_dir)}
    hist = str(tmp_path / "hist.csv")
    _write_histogram(hist, cases["alignment"], which="snp")
    with open(hist, "a") as fh:
        for v in sorted({v for v, _ in cases["few_close"]["close"]} | {v for v, _ in cases["few_close"]["distant"]}):
            fh.write("filter,%d,%d,%d,0,refA\n" % (v, dict(map(tuple, cases["few_close"]["close"])).get(v, 0),
                                                   dict(map(tuple, cases["few_close"]["distant"])).get(v, 0)))
    snp = _run(["--histogram", hist, "-o", str(tmp_path / "a.csv")])
    flt = _run(["--histogram", hist, "--which", "filter", "-o", str(tmp_path / "b.csv")])
    assert snp["snp_threshold"] == cases["alignment"]["snp_threshold"] and flt["snp_threshold"] == cases["few_close"]["snp_threshold"]
    assert snp["n_close"] != flt["n_close"]


def test_errors(golden_dir, tmp_path):
    case = {c["name"]: c for c in _cases(golden_dir)}["few_close"]
    hist, out = str(tmp_path / "hist.csv"), str(tmp_path / "o.csv")
    _write_histogram(hist, case)

    def message(argv):
        with pytest.raises(SystemExit) as e:
            _run(argv)
        assert not os.path.exists(out)
        return str(e.value.code)
    assert "--which must be snp or filter, got 'ek'" in message(["--histogram", hist, "--which", "ek", "-o", out])
    assert "give --close and --distant, or --histogram" in message(["-o", out])
    assert "give --close and --distant, or --histogram" in message(["--close", hist, "-o", out])
    assert "--histogram replaces --close and --distant" in message(["--histogram", hist, "--close", hist, "-o", out])
    # empty classes: a histogram made without --groups has only `ungrouped` counts
    flat = str(tmp_path / "flat.csv")
    with open(flat, "w") as fh:
        fh.write("column,distance,within,between,ungrouped,MSA file\nsnp,3,0,0,10,refA\nsnp,4,0,0,2,refA\n")
    m = message(["--histogram", flat, "-o", out])
    assert "has no pairs in the 'within' column" in m and "--groups" in m
    only_within = str(tmp_path / "w.csv")
    with open(only_within, "w") as fh:
        fh.write("column,distance,within,between,ungrouped,MSA file\nsnp,3,4,0,10,refA\n")
    m = message(["--histogram", only_within, "-o", out])
    assert "has no pairs in the 'between' column" in m and "--groups" in m
    assert "has no pairs in the 'within' column of its 'filter' rows" in message(["--histogram", hist, "--which", "filter", "-o", out])
    bad = str(tmp_path / "bad.csv")
    with open(bad, "w") as fh:
        fh.write("column,distance,within,between,ungrouped,MSA file\nsnp,3,4,1,10,refA\nsnp,x,4,1,10,refA\n")
    assert "%s line 3 is not a histogram row" % bad in message(["--histogram", bad, "-o", out])
    # malformed values in the raw files: file and line are named
    good = str(tmp_path / "good.csv")
    _write_raw(good, case["distant"])
    for k, cell in enumerate(("2.5", "-1", "abc", "", "nan", "1e3", "+3", "1_000", "3.", ".0")):
        raw = str(tmp_path / ("raw%d.csv" % k))
        with open(raw, "w") as fh:
            fh.write("pair,distance\na,3\nb,4.0\nc,%s\n" % cell)
        m = message(["--close", raw, "--distant", good, "-o", out])
        assert "%s line 4" % raw in m and "non-negative integer" in m
        m = message(["--close", good, "--distant", raw, "-o", out])
        assert "%s line 4" % raw in m
    short = str(tmp_path / "short.csv")
    with open(short, "w") as fh:
        fh.write("pair,distance\na,3\nb\n")
    m = message(["--close", short, "--distant", good, "-o", out])
    assert "%s line 3" % short in m and "no such column" in m
    empty = str(tmp_path / "empty.csv")
    with open(empty, "w") as fh:
        fh.write("pair,distance\n")
    assert "--close %s holds no distances" % empty in message(["--close", empty, "--distant", good, "-o", out])


def test_column_option(golden_dir, tmp_path):
    case = {c["name"]: c for c in _cases(golden_dir)}["few_close"]
    for name, h in (("c", case["close"]), ("d", case["distant"])):
        vals = np.repeat([v for v, _ in h], [c for _, c in h])
        with open(str(tmp_path / (name + ".csv")), "w") as fh:
            fh.write("a,b,c,distance\n")
            for v in vals:
                fh.write("s1,s2,99999,%d\n" % v)
    res = _run(["--close", str(tmp_path / "c.csv"), "--distant", str(tmp_path / "d.csv"), "--column", "3", "-o", str(tmp_path / "o.csv")])
    assert res["snp_threshold"] == case["snp_threshold"] and abs(res["lambda"] - case["lambda"]) <= XATOL
    assert _parser().parse_args(["--close", "a", "--distant", "b", "-o", "o"]).column == 1


def test_threshold_is_a_command_now(tmp_path):
    p = subprocess.run([sys.executable, "-m", "tracs_amd", "threshold", "-h"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 0
    assert "not part of the MI355X distance path" not in p.stdout + p.stderr
    assert "--histogram" in p.stdout and "--close" in p.stdout and "--distant" in p.stdout and "--column" in p.stdout
    p = subprocess.run([sys.executable, "-m", "tracs_amd", "-h"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 0 and "threshold" in p.stdout


def test_other_commands_do_not_import_scipy():
    code = ("import sys; sys.argv = ['tracs', 'distance', '-h']\n"
            "import tracs_amd.distance, tracs_amd.threshold, tracs_amd.cluster\n"
            "assert 'scipy' not in sys.modules, 'scipy imported outside the threshold fit'\n")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
