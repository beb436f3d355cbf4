"""Shared by tests/test_gpu_cli_routes_pinned.py and tests/golden/make_cli_routes_golden.py: the inputs, the list of `tracs distance` /
`tracs pair-sites` command lines (every route, each without a rule and under all of them), and the runner that records what a route
wrote and logged.  Nothing here is an expected value: the golden file is written by running these through the package of the commit
BEFORE the host layer moved onto tracs_amd/handle.py."""
import argparse
import hashlib
import io
import logging
import math
import os
import sys

import numpy as np

N, L, N0, K = 24, 700, 10, 3
HEAVY = (3, 17)                        # the two samples that are N on 60 % of the columns: one in each file of the --msa-db cut
CONTIGS = [("ctgA", 400), ("ctgB", 300)]
MASK = [("ctgA", 30, 75), ("ctgA", 120, 131), ("ctgB", 200, 260)]      # the third in the second contig's coordinates: columns 600 .. 659
G, F = 0.5, 0.2                        # --max-sample-n-share, --max-n-share


def make_inputs(td):
    """The files of every route and the thresholds, chosen from the oracle -> dict; nothing here touches the GPU"""
    from oracle import oracle as O
    from tracs_amd import synth
    seqs = synth.alignment(N, L, seed=9091, n_lineages=4, mu_lineage=3e-2, mu_sample=1e-2, p_n=0.04, p_partial=0.01)
    rng = np.random.default_rng(9092)
    for s in HEAVY:
        seqs[s, rng.choice(L, (L * 6) // 10, replace=False)] = ord("N")
    names = ["r%02d" % i for i in range(N)]
    p = lambda name: os.path.join(td, name)                                  # noqa: E731
    inp = dict(td=td, seqs=seqs, names=names, fa=p("routes.fa"), q=p("routes_q.fa"), db=p("routes_db.fa"), meta=p("dates.csv"),
               groups=p("groups.csv"), bed=p("mask.bed"), ref=p("reference.fa"))
    synth.write_fasta(inp["fa"], seqs, names=names, width=60)
    synth.write_fasta(inp["q"], seqs[:N0], names=names[:N0])
    synth.write_fasta(inp["db"], seqs[N0:], names=names[N0:])
    iso, days = synth.dates(N, seed=9093)
    with open(inp["meta"], "w") as fh:
        fh.write("name,date\n" + "".join("%s,%s\n" % (a, b) for a, b in zip(names, iso)))
    inp["labels"] = {nm: ("g%d" % (i % 3) if i % 5 else None) for i, nm in enumerate(names)}
    with open(inp["groups"], "w") as fh:
        fh.write("name,group\n" + "".join("%s,%s\n" % (nm, lab or "") for nm, lab in inp["labels"].items()))
    with open(inp["ref"], "w") as fh:
        fh.write("".join(">%s\n%s\n" % (nm, "A" * n) for nm, n in CONTIGS))
    with open(inp["bed"], "w") as fh:
        fh.write("".join("%s\t%d\t%d\n" % iv for iv in MASK))
    keep = np.ones(L, bool)
    start = {"ctgA": 0, "ctgB": 400}
    for c, s, e in MASK:
        keep[start[c] + s:start[c] + e] = False
    inp["keep"] = keep
    rest = np.ones(N, bool)
    rest[list(HEAVY)] = False
    d = O.pairsnp_arrays(seqs[rest][:, keep])[2]
    inp["dist"] = int(np.sort(d)[len(d) // 2])                               # -D: half of the pairs of the N-light samples
    # -K: the median E(K) of the --msa-db pairs within -D (the oracle's, at the command's default rates): drops some rows, not all
    r, c, d, _ = O.pairsnp_arrays(seqs, n0=N0, dist=inp["dist"])
    years = np.abs(days[r.astype(np.int64)] - days[c.astype(np.int64)]).astype(np.float64) * 86400.0 / 31556952.0
    ek = np.sort(O.trans_dist(d.astype(np.int32), years, 1e-3 * 29903, 73.0, 0.01)[1])
    inp["max_hosts"] = int(ek[len(ek) // 2])
    assert ek[0] < inp["max_hosts"] < ek[-1] - 1
    return inp


def ruled_alignment(inp, isn, share=True):
    """The three rules in their order, in numpy -> (kept samples bool[N], kept columns bool[L], N counts, L')"""
    seqs, keep = inp["seqs"], inp["keep"]
    is_n = isn[seqs]
    lp = int(keep.sum())
    counts = is_n[:, keep].sum(axis=1)
    samples = counts <= math.floor(G * lp)
    cols = keep & (is_n[samples].sum(axis=0) <= math.floor(F * int(samples.sum()))) if share else keep.copy()
    return samples, cols, counts, lp


def min_sites_of(inp, isn):
    """--min-sites: the median compared-sites count of the ruled run's pairs within -D -- vetoes some pairs, not all"""
    from oracle import oracle as O
    samples, cols, _, _ = ruled_alignment(inp, isn)
    nn = O.pairsnp_arrays(inp["seqs"][samples][:, cols], dist=inp["dist"])[3]
    return int(np.sort(nn)[len(nn) // 2])


def max_n_of(inp, isn):
    """Sites(max_n_samples=...) of the API's `sites=` call, from the data: the file-kept columns with the most N go too"""
    return int(isn[inp["seqs"]].sum(axis=0)[inp["keep"]].max()) - 1


def routes(inp, min_sites):
    """[(name, command, options without the outputs, {option: output file name}, environment)] in the order they run"""
    meta = ["--meta", inp["meta"]]
    one, two = ["--msa", inp["fa"]], ["--msa", inp["q"], "--msa-db", inp["db"]]
    base = [("full_meta", one + meta), ("full_nometa", one), ("filter", one + meta + ["--filter"]), ("db_K", two + meta + ["-K", str(inp["max_hosts"])]),
            ("nearest", one + meta + ["--nearest", str(K)]), ("mst", one + meta + ["--mst", "snp"]),
            ("ancestors", one + meta + ["--ancestors", "direct"]), ("histogram", one + ["--histogram", "--groups", inp["groups"]])]
    file_rules = ["--mask", inp["bed"], "--mask-reference", inp["ref"]]
    rules = file_rules + ["--max-n-share", str(F), "--max-sample-n-share", str(G), "--min-sites", str(min_sites)]
    out = []
    for name, opts in base:
        extra = {"--ancestors-out": "tree.csv"} if name == "ancestors" else {}
        out.append((name, "distance", opts, dict(extra), {}))
        outs = dict(extra, **{"--samples-out": "samples.csv"})
        if name != "nearest":                            # (refused: --sites-out with --nearest and --max-n-share)
            outs["--sites-out"] = "sites.bed"
        out.append((name + "_ruled", "distance", opts + rules, outs, {}))
    out.append(("lone_max_n_share", "distance", one + meta + ["--max-n-share", str(F)], {"--sites-out": "sites.bed"}, {}))
    msa_outs = {"--msa-out": "compared.fa", "--site-table": "table.csv"}
    out.append(("msa_out_device", "distance", one + meta + rules, dict(msa_outs, **{"--sites-out": "sites.bed", "--samples-out": "samples.csv"}), {}))
    out.append(("msa_out_nearest", "distance", one + ["--nearest", str(K)] + rules, dict(msa_outs, **{"--samples-out": "samples.csv"}), {}))
    out.append(("arrays_ruled", "distance", one + meta + rules, {"--sites-out": "sites.bed", "--samples-out": "samples.csv"},
                {"TRACS_DISTANCE_ARRAYS": "1"}))
    out.append(("staged", "distance", one + meta + ["--filter"], {}, {"TRACS_STAGE_TRACE": "1"}))
    out.append(("pair_sites_ruled", "pair-sites", one + ["--pairs", os.path.join(inp["td"], "out", "full_meta_ruled", "out.csv"), "--filter"]
                + file_rules + ["--max-n-share", str(F), "--max-sample-n-share", str(G)], {}, {}))
    return out


class _Messages(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.got = []

    def emit(self, record):
        self.got.append(record.getMessage())


def run_route(inp, route):
    """One command line through its parser's func, in this process -> {"files": {name: {sha256, lines}}, "info": [messages],
    "stages": [names]}.  The outputs go to <td>/out/<route>/; the temporary directory is written as {tmp} in the messages."""
    import tracs_amd.distance as di
    import tracs_amd.pair_sites as ps
    name, command, opts, outs, env = route
    folder = os.path.join(inp["td"], "out", name)
    os.makedirs(folder)
    argv = list(opts) + ["-o", os.path.join(folder, "out.csv"), "--loglevel", "INFO"]
    if command == "distance":
        argv += ["-D", str(inp["dist"])]
    for opt, fname in outs.items():
        argv += [opt, os.path.join(folder, fname)]
    parser = {"distance": di.distance_parser, "pair-sites": ps.pair_sites_parser}[command](argparse.ArgumentParser())
    args = parser.parse_args(argv)
    root, handler, err = logging.getLogger(), _Messages(), io.StringIO()
    level, old_err, old_env = root.level, sys.stderr, {k: os.environ.get(k) for k in env}
    root.addHandler(handler)
    root.setLevel(logging.INFO)
    os.environ.update(env)
    if env.get("TRACS_STAGE_TRACE"):
        sys.stderr = err
    try:
        args.func(args)
    finally:
        sys.stderr = old_err
        root.removeHandler(handler)
        root.setLevel(level)
        for k, v in old_env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    files = {}
    for fname in sorted(os.listdir(folder)):
        data = open(os.path.join(folder, fname), "rb").read()
        files[fname] = {"sha256": hashlib.sha256(data).hexdigest(), "lines": data.count(b"\n")}
    # (the "process start" stage line needs an optional module and is left out; the others are the tracer's own)
    stages = [ln[len("[stage] "):].rsplit(" ", 2)[0] for ln in err.getvalue().split("\n")
              if ln.startswith("[stage] ") and not ln.startswith("[stage] process start")]
    return {"files": files, "info": [m.replace(inp["td"], "{tmp}") for m in handler.got], "stages": stages}


def api_calls(inp, min_sites, max_n):
    """name -> (function name, positional arguments after the files, keywords) of the API half: nothing, `sites=` alone, the rule
    keywords"""
    from tracs_amd.sites import Sites
    pairs = [("r00", "r01"), (5, "r20"), ("r23", 2), (7, 8)]
    alone = dict(sites=Sites(inp["keep"], max_n))
    ruled = dict(sites=Sites(inp["keep"]), max_sample_n_share=G, max_n_share=F)
    out = {}
    for fn, head, kw, with_min in (("pairsnp_arrays", (), dict(dist=inp["dist"], filter=True), True),
                                   ("nearest_arrays", (K,), dict(dist=inp["dist"]), True),
                                   ("distance_histogram", (), dict(dist=inp["dist"], groups=inp["labels"]), True),
                                   ("pair_sites", (pairs,), dict(filter=True), False)):
        out[fn + ":nothing"] = (fn, head, dict(kw))
        out[fn + ":sites"] = (fn, head, dict(kw, **alone))
        out[fn + ":rules"] = (fn, head, dict(kw, **ruled, **(dict(min_sites=min_sites) if with_min else {})))
    return out
