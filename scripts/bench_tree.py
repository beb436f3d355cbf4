#!/usr/bin/env python3
"""The neighbour-joining tree on bench.py's workload, or with --method bionj the BIONJ tree.  Prints
one JSON line; --out FILE also writes it there.

    python scripts/bench_tree.py [--samples 10000] [--sites 5000000] [--steps 3] [--warmup 1] [--workload sparse] [--per-site] [--method nj]
    python scripts/bench_tree.py --cli [--samples 10000] [--sites 20000] [--method nj]      # `tracs distance --tree METHOD`, the entry point itself

The alignment is synthesised on the device (synth.pack_synthetic_device, as bench.py does), then each call runs what
tracs_distance_tree runs: row panels of tracs_pairsnp_dense_thr without a threshold (~1 GiB per matrix) -> tracs_nj_load_panel ->
tracs_nj_run -> tracs_nj_emit -> tracs_nj_edges -> tracs_tree_write (Newick and edge rows into a temporary folder).  Reported: the
wall time of the call and of its three stages (the device drained after each): dense panels + load / join loop / emit + write.
The floor of the join loop is what its scans have to read, sum over r = 4 .. n of r (r - 1) / 2 cells of 8 bytes, at the streaming
rate DESIGN.md 3.2 records for classify_sites_kernel; `ratio_to_floor` is the join loop's time over that.  For per-kernel times run
it under `rocprofv3 --kernel-trace --stats`, in a run of its own.
--cli: tracs_distance_tree itself, end to end through `python -m tracs_amd distance --tree nj --tree-edges` under TRACS_STAGE_TRACE on a
lineage-structured FASTA of --samples x --sites written to a temporary folder (the join loop does not depend on the number of sites,
a FASTA of bench.py's shape would be 50 GB): wall time, the library's own three stages and the sizes of the two files.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_BYTES_PER_S = 5.97e12          # classify_sites_kernel: 25.12 GB in 4.23 ms (the faster box)


def cli(args):
    import subprocess

    from tracs_amd import synth
    n, L = args.samples, args.sites
    tmp = tempfile.mkdtemp(prefix="tracs_tree_")
    try:
        seqs = synth.alignment(n, L, seed=5, mu_lineage=2e-3, mu_sample=5e-4, n_lineages=20, p_n=0.01)
        fa = os.path.join(tmp, "bench_combined.fasta")
        synth.write_fasta(fa, seqs, names=["sample_%05d" % i for i in range(n)])
        del seqs
        nwk, edges = os.path.join(tmp, "t.nwk"), os.path.join(tmp, "e.csv")
        t0 = time.perf_counter()
        rc = subprocess.run([sys.executable, "-m", "tracs_amd", "distance", "--msa", fa, "--tree", args.method, "-o", nwk, "--tree-edges", edges,
                             "--loglevel", "ERROR"], cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, TRACS_STAGE_TRACE="1"))
        dt = time.perf_counter() - t0
        if rc.returncode != 0:
            raise SystemExit(rc.stderr[-3000:])
        import re
        stages = {}
        for line in rc.stderr.splitlines():
            m = re.match(r"\[stage\] (.*?) ([0-9.]+) s( \(.*\))?$", line)
            if m:
                stages[m.group(1)] = float(m.group(2))
        with open(edges) as fh:
            rows = sum(1 for _ in fh) - 1
        import hashlib
        with open(nwk, "rb") as fh:
            digest = hashlib.sha256(fh.read()).hexdigest()
        out = dict(metric="tree_cli_s", value=dt, unit="s", higher_is_better=False, n=n, L=L, method=args.method, stages_s=stages, edge_rows=rows,
                   panel_rows=os.environ.get("TRACS_FOREST_PANEL_ROWS"), newick_bytes=os.path.getsize(nwk),
                   edges_bytes=os.path.getsize(edges), newick_sha256=digest)
        line = json.dumps(out)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=5000000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="sparse")
    ap.add_argument("--per-site", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--method", choices=["nj", "bionj"], default="nj")
    args = ap.parse_args()
    if args.cli:
        return cli(args)
    import numpy as np
    import torch

    from bench import synth_kw
    from tracs_amd import _lib
    from tracs_amd import device as dev
    from tracs_amd import synth
    n, L = args.samples, args.sites
    aln = dev.Alignment(n, L)
    synth.pack_synthetic_device(aln, seed=20241022 + 2, **synth_kw(0.0, args.workload))
    torch.cuda.synchronize()
    panel = max(64, min(n, (1 << 28) // n))
    d = torch.empty((panel, n), dtype=torch.int32, device="cuda")
    nn = torch.empty_like(d)
    names = ["sample_%05d" % i for i in range(n)]
    cnames = (C.c_char_p * n)(*[x.encode() for x in names])
    lib = _lib.load()
    state_bytes = (lib.tracs_bionj_state_bytes if args.method == "bionj" else lib.tracs_nj_state_bytes)(n)
    tmp = tempfile.mkdtemp(prefix="tracs_tree_")

    def call():
        t = [time.perf_counter()]
        state = dev.nj_init(n, method=args.method)
        for r0 in range(0, n, panel):
            r1 = min(n, r0 + panel)
            dev.pairsnp_dense(aln, d, nn, row_begin=r0, row_end=r1, dist_threshold=2147483647, base_row=r0)
            dev.nj_load_panel(state, n, d, nn, row_begin=r0, row_end=r1, per_site=args.per_site, base_row=r0)
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        (dev.bionj_run if args.method == "bionj" else dev.nj_run)(state, n)
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        parent, child, length = dev.nj_edges(n, *dev.nj_emit(state, n))
        nwk, edges = os.path.join(tmp, "t.nwk"), os.path.join(tmp, "e.csv")
        for p in (nwk, edges):
            open(p, "w").close()
        _lib.check(lib.tracs_tree_write(cnames, n, parent.ctypes.data, child.ctypes.data, length.ctypes.data, len(parent), os.fsencode(nwk),
                                        b"bench", os.fsencode(edges)))
        t.append(time.perf_counter())
        return [b - a for a, b in zip(t[:-1], t[1:])], (os.path.getsize(nwk), os.path.getsize(edges), int((length < 0).sum()))

    try:
        for _ in range(args.warmup):
            call()
        runs = [call() for _ in range(args.steps)]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    stages = np.array([r[0] for r in runs])
    med = np.median(stages, axis=0)
    total = np.median(stages.sum(axis=1))
    floor_bytes = sum(r * (r - 1) // 2 * 8 for r in range(4, n + 1))
    floor_s = floor_bytes / STREAM_BYTES_PER_S
    out = dict(metric="tree_call_s", value=float(total), unit="s", higher_is_better=False, n=n, L=L, workload=args.workload, method=args.method,
               state_bytes=int(state_bytes), per_site=bool(args.per_site), steps=args.steps, warmup=args.warmup, panel_rows=panel,
               dense_panels_and_load_s=float(med[0]), join_loop_s=float(med[1]), emit_and_write_s=float(med[2]),
               stage_s=[[float(x) for x in row] for row in stages], joins=max(n - 3, 0), launches=3 * max(n - 3, 0) + 2,
               scan_floor_bytes=floor_bytes, stream_bytes_per_s=STREAM_BYTES_PER_S, scan_floor_s=floor_s,
               ratio_to_floor=float(med[1] / floor_s) if floor_s else None, join_loop_us_per_join=float(med[1] / max(n - 3, 1) * 1e6),
               newick_bytes=runs[-1][1][0], edges_bytes=runs[-1][1][1], negative_lengths=runs[-1][1][2])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
