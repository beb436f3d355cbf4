#!/usr/bin/env python3
"""k nearest neighbours per sample on bench.py's workload.  Prints one JSON line.

    python scripts/bench_nearest.py [--samples 10000] [--sites 5000000] [--k 16] [--steps 5] [--warmup 1] [--workload sparse]
    python scripts/bench_nearest.py --cli --sites 500000 [--k 10]      # `tracs distance --nearest K` next to the all-pairs run

The alignment is synthesised on the device (synth.pack_synthetic_device, as bench.py does: a FASTA of 10 000 x 5 Mbp would be 50 GB),
then each call runs what tracs_nearest runs after its FASTA read: row panels of tracs_pairsnp_dense_thr (~1 GiB per matrix) ->
tracs_knn_update -> tracs_knn_emit -> the lists copied to the host.  Reported: the wall time per call, and from CUDA events on the
resident panel the dense pass alone and the selection alone (update + emit, on a fresh state each time), so that selection / dense is
the share of the call's kernel time the selection takes.  For per-kernel times run it under `rocprofv3 --kernel-trace --stats`.
--cli: end to end through `python -m tracs_amd distance` with dates, on a lineage-structured FASTA of --samples x --sites written to a
temporary folder: wall time and CSV size of the all-pairs run and of --nearest K, in the same process tree, one after the other.
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
    tmp = tempfile.mkdtemp(prefix="tracs_nearest_")
    try:
        seqs = synth.alignment(n, L, seed=5, mu_lineage=2e-4, mu_sample=2e-5, n_lineages=20, p_n=0.01)
        names = ["sample_%05d" % i for i in range(n)]
        fa = os.path.join(tmp, "bench_combined.fasta")
        synth.write_fasta(fa, seqs, names=names)
        del seqs
        iso, _ = synth.dates(n, seed=6)
        meta = os.path.join(tmp, "dates.csv")
        with open(meta, "w") as f:
            f.write("sample,date\n")
            for a, b in zip(names, iso):
                f.write("%s,%s\n" % (a, b))
        out = dict(metric="nearest_cli_s", unit="s", higher_is_better=False, n=n, L=L, k=args.k)
        for label, extra in (("all_pairs", []), ("nearest", ["--nearest", str(args.k)])):
            csv = os.path.join(tmp, label + ".csv")
            t0 = time.perf_counter()
            rc = subprocess.run([sys.executable, "-m", "tracs_amd", "distance", "--msa", fa, "--meta", meta, "-o", csv, "--loglevel", "ERROR"]
                                + extra, cwd=ROOT, capture_output=True, text=True)
            dt = time.perf_counter() - t0
            if rc.returncode != 0:
                raise SystemExit(rc.stderr[-3000:])
            with open(csv, "rb") as fh:
                rows = sum(1 for _ in fh) - 1
            out[label] = {"s": dt, "rows": rows, "csv_MB": os.path.getsize(csv) / 1e6}
            os.remove(csv)
        out["value"] = out["nearest"]["s"]
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=5000000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="sparse")
    ap.add_argument("--cli", action="store_true")
    args = ap.parse_args()
    if args.cli:
        return cli(args)
    import torch

    from bench import synth_kw
    from tracs_amd import device as dev
    from tracs_amd import synth
    n, L, k = args.samples, args.sites, args.k
    aln = dev.Alignment(n, L)
    synth.pack_synthetic_device(aln, seed=20241022 + 2, **synth_kw(0.0, args.workload))
    torch.cuda.synchronize()
    panel = max(64, min(n, (1 << 28) // n))
    d = torch.empty((panel, n), dtype=torch.int32, device="cuda")
    nn = torch.empty_like(d)
    thr = 2147483647

    def call(select=True):
        state = dev.knn_init(n, k) if select else None
        for r0 in range(0, n, panel):
            r1 = min(n, r0 + panel)
            dev.pairsnp_dense(aln, d, nn, row_begin=r0, row_end=r1, dist_threshold=thr, base_row=r0)
            if select:
                dev.knn_update(state, d, nn, n, k, row_begin=r0, row_end=r1, dist_threshold=thr, base_row=r0)
        if select:
            return [t.cpu() for t in dev.knn_emit(state, k, 0, n)]
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
    emitted = int(out[0].numel())

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

    dense_ms = events(lambda: call(select=False), args.steps)
    sel = {}
    if panel >= n:                                          # the whole matrix is one resident panel: time the selection on it alone
        def select_only():
            state = dev.knn_init(n, k)
            dev.knn_update(state, d, nn, n, k, dist_threshold=thr)
            dev.knn_emit(state, k, 0, n)
        sel["select_ms"] = events(select_only, args.steps)
        sel["select_share_of_dense"] = sel["select_ms"] / dense_ms
    wall.sort()
    print(json.dumps(dict(metric="nearest_call_ms", value=wall[len(wall) // 2], unit="ms", higher_is_better=False, n=n, L=L, k=k,
                          workload=args.workload, steps=args.steps, warmup=args.warmup, panel_rows=panel, pairs_emitted=emitted,
                          wall_ms=wall, dense_ms=dense_ms, **sel)))


if __name__ == "__main__":
    main()
