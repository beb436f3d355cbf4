"""The row-panel walk and the pair-extraction stage of the host entry points (csrc/capi.hip: PanelWalk, PairStage) on the routes
every user takes -- `tracs distance` full output, the array route, --nearest, --histogram --filter -- across panel seams: 47 samples
at 7 rows and at 1 row per panel (TRACS_FOREST_PANEL_ROWS), the last panel ragged, one whole panel without a pair, the pair buffers
regrown, device-to-host batches of 64 rows that end inside a panel.  Three pins: the same bytes at every panel height; the integer
columns equal to the CPU oracle; the CSV files equal to what the library wrote BEFORE the entry points shared one walk
(tests/golden/panel_walk_golden.json, written by tests/golden/make_panel_walk_golden.py from a build of that commit).  The --mst and
--ancestors routes (u32, f64 ascending and f64 descending keys) were added with csrc/pair_select.h: their entries come from a build of
commit 27c4601, the last one in which forest.hip and ancestors.hip each carried their own primitives; regenerating the file from that
build reproduced the eight older entries unchanged."""
import argparse
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, L, D, N0, K = 47, 3000, 20, 30, 3
QUIET = range(14, 21)                    # at 7 rows per panel these are one panel; far from every sample: it emits no pair
HEIGHTS = (None, "7", "1")               # None: the default height, one panel at this size
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "panel_walk_golden.json")


def make_inputs(td):
    """The alignment (one file, and cut 30 + 17 for --msa-db), the dates and the oracle's pairs within the threshold.
    -> dict; nothing here touches the GPU."""
    from oracle import oracle as O
    from tracs_amd import synth
    seqs = synth.alignment(N, L, seed=4747, n_lineages=3, mu_lineage=1e-2, mu_sample=1e-3, p_n=0.02, p_partial=0.002)
    rng = np.random.default_rng(4748)
    step = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}
    for s in QUIET:                      # ~50 private substitutions each
        for p in rng.choice(L, 50, replace=False):
            seqs[s, p] = step.get(int(seqs[s, p]), int(seqs[s, p]))
    names = ["w%02d" % i for i in range(N)]
    inp = dict(seqs=seqs, names=names, fa=os.path.join(td, "walk.fa"), q=os.path.join(td, "walkq.fa"), db=os.path.join(td, "walkdb.fa"),
               meta=os.path.join(td, "dates.csv"))
    synth.write_fasta(inp["fa"], seqs, names=names)
    synth.write_fasta(inp["q"], seqs[:N0], names=names[:N0])
    synth.write_fasta(inp["db"], seqs[N0:], names=names[N0:])
    iso, _ = synth.dates(N, seed=4749)
    with open(inp["meta"], "w") as fh:
        fh.write("name,date\n" + "".join("%s,%s\n" % (a, b) for a, b in zip(names, iso)))
    inp["one"] = O.pairsnp_arrays(seqs, dist=D, n_threads=4)
    inp["two"] = O.pairsnp_arrays(seqs, n0=N0, dist=D, n_threads=4)
    # --min-sites: the median of the compared-sites counts of the pairs within the threshold -- vetoes some pairs, not all
    inp["min_sites"] = int(np.sort(inp["one"][3])[len(inp["one"][3]) // 2])
    return inp


def csv_routes(inp):
    """name -> the `tracs distance` options after --msa ... -o ..., for every route that writes a CSV"""
    meta = ["--meta", inp["meta"]]
    one, two = ["--msa", inp["fa"]], ["--msa", inp["q"], "--msa-db", inp["db"]]
    return {"full_meta": one + meta, "full_nometa": one, "full_meta_filter": one + meta + ["--filter"],
            "full_db": two + meta + ["-K", "300"], "full_min_sites": one + meta + ["--min-sites", str(inp["min_sites"])],
            "nearest": one + ["--nearest", str(K)], "nearest_db": two + ["--nearest", str(K)],
            "histogram_filter": one + ["--histogram", "--filter"],
            "mst_snp": one + meta + ["--mst", "snp"], "mst_expectedK": one + meta + ["--mst", "expectedK"],
            "ancestors_snp": one + meta + ["--ancestors", "snp"], "ancestors_direct": one + meta + ["--ancestors", "direct"]}


def run_routes(inp, td, height):
    """Every route once at the given panel height (None: default), in this process.  -> {name: CSV bytes}, {name: arrays}"""
    from tracs_amd import api
    from tracs_amd import distance as di
    env = {"TRACS_FOREST_PANEL_ROWS": height, "TRACS_DISTANCE_BATCH_ROWS": "64"}
    old = {k: os.environ.get(k) for k in env}
    csv, arrays = {}, {}
    try:
        for k, v in env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        for name, opts in csv_routes(inp).items():
            out = os.path.join(td, "%s_%s.csv" % (name, height or "default"))
            args = di.distance_parser(argparse.ArgumentParser()).parse_args(opts + ["-o", out, "-D", str(D), "--loglevel", "ERROR"])
            args.func(args)
            with open(out, "rb") as fh:
                csv[name] = fh.read()
        # (copies: the arrays that come back are views of a result that lives only as long as they do)
        r, c, d, _, f, nn = api.pairsnp_arrays([inp["fa"]], dist=D, filter=True)
        arrays["pairsnp_filter"] = [np.array(x, np.uint64) for x in (r, c, d, nn, f)]
        r, c, d, _, f, nn = api.nearest_arrays([inp["fa"]], K, dist=D)
        arrays["nearest"] = [np.array(x, np.uint64) for x in (r, c, d, nn)]
        r, c, d, _, f, nn = api.nearest_arrays([inp["q"], inp["db"]], K, dist=D)
        arrays["nearest_db"] = [np.array(x, np.uint64) for x in (r, c, d, nn)]
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return csv, arrays


def digest(csv):
    """what the golden file holds of a CSV"""
    return {"sha256": hashlib.sha256(csv).hexdigest(), "rows": csv.count(b"\n") - 1}


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return make_inputs(str(tmp_path_factory.mktemp("panel_walk")))


@pytest.fixture(scope="module")
def runs(hiplib, inputs, tmp_path_factory):
    td = str(tmp_path_factory.mktemp("panel_walk_out"))
    return {h: run_routes(inputs, td, h) for h in HEIGHTS}


def test_one_panel_emits_nothing_and_later_ones_do(inputs):
    """from the oracle alone, before anything runs: rows 14 ... 20 have no j > i within the threshold (nor a database partner), the rows
    after them have; seven panels at height 7, the last one ragged"""
    for r, _, _, _ in (inputs["one"], inputs["two"]):
        r = r.astype(np.int64)
        assert not np.isin(r, list(QUIET)).any()
        assert (r > QUIET[-1]).any() and (r < QUIET[0]).any()
    assert N % 7 == 5 and (N + 6) // 7 == 7 and QUIET[0] % 7 == 0 and len(QUIET) == 7
    nn = inputs["one"][3]
    assert (nn < inputs["min_sites"]).any() and (nn >= inputs["min_sites"]).any()
    assert len(inputs["one"][0]) > 64                    # more than one device-to-host batch


@pytest.mark.parametrize("height", HEIGHTS[1:])
def test_same_bytes_at_every_panel_height(runs, height):
    csv0, arr0 = runs[None]
    csv, arr = runs[height]
    for name in csv0:
        assert csv[name] == csv0[name], (name, height)
    for name in arr0:
        for a, b in zip(arr[name], arr0[name]):
            assert np.array_equal(a, b), (name, height)


def parse_rows(csv, names):
    """-> i, j, d, compared sites as int64 arrays, and the filtered column as text"""
    idx = {nm: k for k, nm in enumerate(names)}
    rows = [ln.split(",") for ln in csv.decode().strip().split("\n")[1:]]
    cols = [np.array([idx[f[0]] for f in rows], np.int64), np.array([idx[f[1]] for f in rows], np.int64),
            np.array([int(f[3]) for f in rows], np.int64), np.array([int(f[7]) for f in rows], np.int64)]
    return cols, [f[6] for f in rows]


def same(got, exp, what):
    for k, (g, e) in enumerate(zip(got, exp)):
        g, e = np.asarray(g).astype(np.int64), np.asarray(e).astype(np.int64)
        assert g.shape == e.shape and np.array_equal(g, e), (what, k, g.shape, e.shape)


@pytest.mark.parametrize("height", HEIGHTS)
def test_integer_columns_equal_the_oracle(runs, inputs, oracle, height):
    from test_gpu_histogram import bincount_hist
    from test_gpu_nearest import expected as nearest_expected
    csv, arr = runs[height]
    seqs, names = inputs["seqs"], inputs["names"]
    one, two = inputs["one"], inputs["two"]
    filt = oracle.filter_recomb_pairs(seqs, one[0], one[1], n_threads=4)
    got, f = parse_rows(csv["full_meta"], names)
    same(got, one, "full_meta")
    assert set(f) == {"NA"}
    got, f = parse_rows(csv["full_nometa"], names)
    same(got, one, "full_nometa")
    assert set(f) == {"0"}
    got, f = parse_rows(csv["full_meta_filter"], names)
    same(got, one, "full_meta_filter")
    same([np.array([int(x) for x in f])], [filt], "full_meta_filter: filtered d")
    keep = one[3] >= inputs["min_sites"]
    same(parse_rows(csv["full_min_sites"], names)[0], [x[keep] for x in one], "full_min_sites")
    # -K drops rows by E(K): what is written is the oracle's pairs in their order, less the dropped ones
    got, _ = parse_rows(csv["full_db"], names)
    pos = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(two[0], two[1]))}
    at = np.array([pos[(int(a), int(b))] for a, b in zip(got[0], got[1])], np.int64)
    assert len(at) and (np.diff(at) > 0).all()
    same(got, [x[at] for x in two], "full_db")
    same(arr["pairsnp_filter"], list(one) + [filt], "pairsnp_arrays(filter=True)")
    same(arr["nearest"], nearest_expected(oracle, seqs, K, dist=D), "nearest_arrays")
    same(arr["nearest_db"], nearest_expected(oracle, seqs, K, n0=N0, dist=D), "nearest_arrays, two files")
    same(parse_rows(csv["nearest"], names)[0], arr["nearest"], "--nearest")
    same(parse_rows(csv["nearest_db"], names)[0], arr["nearest_db"], "--nearest --msa-db")
    hist = {"snp": [], "filter": []}
    for ln in csv["histogram_filter"].decode().strip().split("\n")[1:]:
        f = ln.split(",")
        hist[f[0]].append([int(x) for x in f[1:5]])
    ungrouped = np.full(len(one[0]), 2, np.int64)
    for column, values in (("snp", one[2]), ("filter", filt)):
        same(np.array(hist[column], np.int64).T, bincount_hist(values, ungrouped), "--histogram --filter: " + column)


def test_csv_files_equal_the_parent_commits(runs):
    """the refactors' own pin: sha256 and row count of every CSV as the library wrote them before the entry points shared one walk
    (--mst, --ancestors: before the selection states shared csrc/pair_select.h)"""
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    csv, _ = runs[None]
    assert sorted(golden) == sorted(csv)
    for name in csv:
        assert digest(csv[name]) == golden[name], name
