#!/usr/bin/env python3
"""Each sample's most likely earlier source on bench.py's workload.  Prints one JSON line.

    python scripts/bench_ancestors.py [--samples 10000] [--sites 5000000] [--dist 2147483647] [--steps 5] [--warmup 1] [--workload sparse]
    python scripts/bench_ancestors.py --cli --sites 500000      # `tracs distance --ancestors snp` next to the full run and --mst snp

The alignment is synthesised on the device (synth.pack_synthetic_device, as bench.py does) and every sample gets a sampling day
(synth.dates).  Each call runs what tracs_distance_ancestors runs for `--ancestors snp` apart from the transmission model: row panels
of tracs_pairsnp_dense_thr (~1 GiB per matrix) -> the panel's pairs within -D as COO (tracs_coo_count / fill) ->
tracs_anc_update_coo -> tracs_anc_emit -> links and trees copied to the host.  Reported: the wall time per call, and from CUDA events on
the resident panel the dense pass alone, the COO extraction alone, the ancestor update alone (a fresh state each time) and its emit; the
forest update and emit (tracs_msf_*) on the same pairs in the same process are the yardstick.  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats`.
--cli: end to end through `python -m tracs_amd distance` with dates, on a lineage-structured FASTA of --samples x --sites written to a
temporary folder: wall time and CSV size of the full run, of --mst snp and of --ancestors snp (with --ancestors-out), one after the
other.
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
    tmp = tempfile.mkdtemp(prefix="tracs_ancestors_")
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
        out = dict(metric="ancestors_cli_s", unit="s", higher_is_better=False, n=n, L=L)
        tree = os.path.join(tmp, "tree.csv")
        for label, extra in (("all_pairs", []), ("mst_snp", ["--mst", "snp"]), ("ancestors_snp", ["--ancestors", "snp", "--ancestors-out", tree])):
            csv = os.path.join(tmp, label + ".csv")
            t0 = time.perf_counter()
            rc = subprocess.run([sys.executable, "-m", "tracs_amd", "distance", "--msa", fa, "--meta", meta, "-o", csv, "--loglevel", "ERROR"]
                                + extra, cwd=ROOT, capture_output=True, text=True)
            dt = time.perf_counter() - t0
            if rc.returncode != 0:
                raise SystemExit(rc.stderr[-3000:])
            with open(csv, "rb") as fh:
                rows = sum(1 for _ in fh) - 1
            out[label] = {"s": dt, "rows": rows, "csv_bytes": os.path.getsize(csv)}
            os.remove(csv)
        out["ancestors_snp"]["tree_bytes"] = os.path.getsize(tree)
        out["value"] = out["ancestors_snp"]["s"]
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=5000000)
    ap.add_argument("--dist", type=int, default=2147483647)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="sparse")
    ap.add_argument("--cli", action="store_true")
    args = ap.parse_args()
    if args.cli:
        return cli(args)
    import torch

    from bench import synth_kw
    from tracs_amd import _lib
    from tracs_amd import device as dev
    from tracs_amd import synth
    n, L, thr = args.samples, args.sites, args.dist
    aln = dev.Alignment(n, L)
    synth.pack_synthetic_device(aln, seed=20241022 + 2, **synth_kw(0.0, args.workload))
    _, days_np = synth.dates(n, seed=6)
    days = torch.from_numpy(days_np).cuda()
    torch.cuda.synchronize()
    panel = max(64, min(n, (1 << 28) // n))
    d = torch.empty((panel, n), dtype=torch.int32, device="cuda")
    nn = torch.empty_like(d)

    def call():
        state = dev.anc_init(n, days)
        offered = 0
        for r0 in range(0, n, panel):
            r1 = min(n, r0 + panel)
            dev.pairsnp_dense(aln, d, nn, row_begin=r0, row_end=r1, dist_threshold=thr, base_row=r0)
            r, c, dd, m = dev.coo_from_dense(d, nn, n, dist_threshold=thr, row_begin=r0, row_end=r1, base_row=r0)
            offered += dev.anc_update(state, n, r, c, dd, d=dd, nn=m)
            del r, c, dd, m
        return [t.cpu() for t in dev.anc_emit(state, n)], offered

    for _ in range(args.warmup + 1):
        out, offered = call()
    wall = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, offered = call()
        wall.append((time.perf_counter() - t0) * 1e3)

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

    def dense_only():
        for r0 in range(0, n, panel):
            dev.pairsnp_dense(aln, d, nn, row_begin=r0, row_end=min(n, r0 + panel), dist_threshold=thr, base_row=r0)
    dense_ms = events(dense_only, args.steps)
    parts = {}
    if panel >= n:                                          # the whole matrix is one resident panel: time its stages alone
        dense_only()
        parts["coo_ms"] = events(lambda: dev.coo_from_dense(d, nn, n, dist_threshold=thr), args.steps)
        coo = dev.coo_from_dense(d, nn, n, dist_threshold=thr)
        st = {}

        def anc_update_only():
            st["anc"] = dev.anc_init(n, days)
            dev.anc_update(st["anc"], n, coo[0], coo[1], coo[2], d=coo[2], nn=coo[3])

        def forest_update_only():
            st["msf"] = dev.msf_init(n)
            dev.msf_update(st["msf"], n, coo[0], coo[1], coo[2], d=coo[2], nn=coo[3])
        # the two updates alternate, so that a drift of the box shows in both
        a_ms, f_ms = [], []
        for _ in range(2):
            anc_update_only()
            forest_update_only()
        for _ in range(max(args.steps, 3)):
            a_ms.append(events(anc_update_only, 1))
            f_ms.append(events(forest_update_only, 1))
        a_ms.sort()
        f_ms.sort()
        parts["anc_update_ms"] = a_ms[len(a_ms) // 2]
        parts["forest_update_ms"] = f_ms[len(f_ms) // 2]
        parts["anc_update_ms_all"] = a_ms
        parts["forest_update_ms_all"] = f_ms
        parts["anc_emit_ms"] = events(lambda: dev.anc_emit(st["anc"], n), args.steps)
        parts["forest_emit_ms"] = events(lambda: dev.msf_emit(st["msf"], n), args.steps)
        parts["anc_update_share_of_dense"] = parts["anc_update_ms"] / dense_ms
        parts["anc_update_over_forest_update"] = parts["anc_update_ms"] / parts["forest_update_ms"]
    wall.sort()
    L_ = _lib.load()
    print(json.dumps(dict(metric="ancestors_call_ms", value=wall[len(wall) // 2], unit="ms", higher_is_better=False, n=n, L=L, dist=thr,
                          workload=args.workload, steps=args.steps, warmup=args.warmup, panel_rows=panel, candidates_offered=offered,
                          links=int(out[0].numel()), roots=int((out[7] < 0).sum()), max_generation=int(out[9].max()),
                          state_bytes=int(L_.tracs_anc_state_bytes(n)), forest_state_bytes=int(L_.tracs_msf_state_bytes(n)),
                          wall_ms=wall, dense_ms=dense_ms, **parts)))


if __name__ == "__main__":
    main()
