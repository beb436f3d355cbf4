#!/usr/bin/env python3
"""SNP distance histogram on bench.py's workload.  Prints one JSON line.

    python scripts/bench_histogram.py [--samples 10000] [--sites 5000000] [--groups 100] [--steps 5] [--warmup 1] [--workload sparse]
    python scripts/bench_histogram.py --cli --sites 500000      # `tracs distance --histogram` and `tracs threshold` next to the all-pairs run

The alignment is synthesised on the device (synth.pack_synthetic_device, as bench.py does), then each call runs what
tracs_distance_histogram runs after its FASTA read: row panels of tracs_pairsnp_dense_thr (~1 GiB per matrix) -> tracs_hist_update ->
tracs_hist_emit -> the non-empty bins copied to the host.  Reported: the wall time per call, and from CUDA events on the resident panel
the dense pass alone and the histogram alone (init + update + emit on a fresh state each time), without labels and with --groups random
labels, so that hist / dense is the share of the call's kernel time the histogram takes; and the same update on a panel whose cells are
all 0 (10 000 identical samples: every pair in one bin, the contention worst case).  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats`.
--cli: end to end through `python -m tracs_amd`, on a lineage-structured FASTA of --samples x --sites written to a temporary folder:
wall time and output size of the all-pairs run (with dates, as scripts/bench_forest.py --cli runs it), of `distance --histogram --groups` and of `threshold --histogram`, one after the other.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cli(args):
    import shutil
    import subprocess
    import tempfile

    from tracs_amd import synth
    n, L = args.samples, args.sites
    tmp = tempfile.mkdtemp(prefix="tracs_histogram_")
    try:
        n_lin = 20
        seqs = synth.alignment(n, L, seed=5, mu_lineage=2e-4, mu_sample=2e-5, n_lineages=n_lin, p_n=0.01)
        names = ["sample_%05d" % i for i in range(n)]
        fa = os.path.join(tmp, "bench_combined.fasta")
        synth.write_fasta(fa, seqs, names=names)
        del seqs
        groups = os.path.join(tmp, "groups.csv")
        with open(groups, "w") as f:
            f.write("sample,group\n")
            for i, a in enumerate(names):
                f.write("%s,g%d\n" % (a, i % args.groups))
        iso, _ = synth.dates(n, seed=6)
        meta = os.path.join(tmp, "dates.csv")
        with open(meta, "w") as f:
            f.write("sample,date\n")
            for a, b in zip(names, iso):
                f.write("%s,%s\n" % (a, b))
        out = dict(metric="histogram_cli_s", unit="s", higher_is_better=False, n=n, L=L, groups=args.groups)
        hist = os.path.join(tmp, "histogram.csv")
        runs = (("all_pairs", ["distance", "--msa", fa, "--meta", meta, "-o", os.path.join(tmp, "all_pairs.csv")]),
                ("histogram", ["distance", "--msa", fa, "-o", hist, "--histogram", "--groups", groups]),
                ("threshold", ["threshold", "--histogram", hist, "-o", os.path.join(tmp, "threshold.csv")]))
        for label, argv in runs:
            t0 = time.perf_counter()
            rc = subprocess.run([sys.executable, "-m", "tracs_amd"] + argv + (["--loglevel", "ERROR"] if argv[0] == "distance" else []),
                                cwd=ROOT, capture_output=True, text=True)
            dt = time.perf_counter() - t0
            path = argv[argv.index("-o") + 1]
            if rc.returncode != 0:
                out[label] = {"s": dt, "error": rc.stderr[-500:]}
                continue
            with open(path, "rb") as fh:
                rows = sum(1 for _ in fh) - 1
            out[label] = {"s": dt, "rows": rows, "MB": os.path.getsize(path) / 1e6}
            if label == "threshold":
                out[label]["result"] = dict(ln.split(",") for ln in open(path).read().strip().split("\n")[1:])
            if label == "all_pairs":
                os.remove(path)
        out["value"] = out["histogram"]["s"]
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=5000000)
    ap.add_argument("--groups", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="sparse")
    ap.add_argument("--cli", action="store_true")
    args = ap.parse_args()
    if args.cli:
        return cli(args)
    import numpy as np
    import torch

    from bench import synth_kw
    from tracs_amd import device as dev
    from tracs_amd import synth
    n, L = args.samples, args.sites
    aln = dev.Alignment(n, L)
    synth.pack_synthetic_device(aln, seed=20241022 + 2, **synth_kw(0.0, args.workload))
    torch.cuda.synchronize()
    panel = max(64, min(n, (1 << 28) // n))
    d = torch.empty((panel, n), dtype=torch.int32, device="cuda")
    nn = torch.empty_like(d)
    thr = 2147483647
    n_bins = L + 1
    labels = torch.from_numpy(np.random.default_rng(1).integers(0, args.groups, n).astype(np.int32)).cuda()

    def call(group=None, hist=True):
        state = dev.hist_init(n_bins) if hist else None
        for r0 in range(0, n, panel):
            r1 = min(n, r0 + panel)
            dev.pairsnp_dense(aln, d, nn, row_begin=r0, row_end=r1, dist_threshold=thr, base_row=r0)
            if hist:
                dev.hist_update(state, n_bins, d, n, row_begin=r0, row_end=r1, dist_threshold=thr, group=group, base_row=r0)
        if hist:
            return [t.cpu() for t in dev.hist_emit(state, n_bins)]
        torch.cuda.synchronize()
        return None

    for _ in range(args.warmup + 1):
        out = call()
    wall = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t0) * 1e3)
    bins = int(out[0].numel())
    pairs = int(sum(int(t.sum()) for t in out[1:]))
    lo, hi = int(out[0].min()), int(out[0].max())

    def events(fn, reps):
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return sorted(ms)[len(ms) // 2]

    dense_ms = events(lambda: call(hist=False), args.steps)
    res = {}
    if panel >= n:                                          # the whole matrix is one resident panel: time the histogram on it alone
        def hist_only(src, group, bins_, emit=True, init=True):
            def fn():
                state = dev.hist_init(bins_) if init else hist_only.state
                dev.hist_update(state, bins_, src, n, dist_threshold=thr, group=group)
                if emit:
                    dev.hist_emit(state, bins_)
            return fn
        hist_only.state = dev.hist_init(n_bins)
        res["hist_ms"] = events(hist_only(d, None, n_bins), args.steps)
        res["hist_groups_ms"] = events(hist_only(d, labels, n_bins), args.steps)
        res["update_only_ms"] = events(hist_only(d, None, n_bins, emit=False, init=False), args.steps)
        res["update_only_groups_ms"] = events(hist_only(d, labels, n_bins, emit=False, init=False), args.steps)
        res["hist_share_of_dense"] = res["hist_ms"] / dense_ms
        res["hist_groups_share_of_dense"] = res["hist_groups_ms"] / dense_ms
        routes = dev.hist_routes(hist_only.state)
        tot = max(1, routes["combined"] + routes["lds"] + routes["global"])
        res["routes_share"] = {k: routes[k] / tot for k in ("combined", "lds", "global")}
        d.zero_()                                           # 10 000 identical samples: every pair in bin 0
        hist_only.state = dev.hist_init(n_bins)
        res["one_bin_update_only_ms"] = events(hist_only(d, None, n_bins, emit=False, init=False), args.steps)
        res["one_bin_update_only_groups_ms"] = events(hist_only(d, labels, n_bins, emit=False, init=False), args.steps)
        res["one_bin_over_typical"] = res["one_bin_update_only_ms"] / res["update_only_ms"]
        res["one_bin_over_typical_groups"] = res["one_bin_update_only_groups_ms"] / res["update_only_groups_ms"]
    wall.sort()
    print(json.dumps(dict(metric="histogram_call_ms", value=wall[len(wall) // 2], unit="ms", higher_is_better=False, n=n, L=L,
                          groups=args.groups, workload=args.workload, steps=args.steps, warmup=args.warmup, panel_rows=panel,
                          non_empty_bins=bins, pairs_counted=pairs, d_min=lo, d_max=hi,
                          grid=os.environ.get("TRACS_HIST_GRID", "default"),
                          wall_ms=wall, dense_ms=dense_ms, **res)))


if __name__ == "__main__":
    main()
