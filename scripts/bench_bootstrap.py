#!/usr/bin/env python3
"""Bootstrap replicates of the neighbour-joining tree on bench.py's workload.  Prints one JSON line; --out FILE also
writes it there.

    python scripts/bench_bootstrap.py [--samples 10000] [--sites 5000000] [--replicates 8] [--steps 3] [--warmup 1] [--workload sparse]
    python scripts/bench_bootstrap.py --cli [--samples 10000] [--sites 5000] [--replicates 8]      # the entry point itself

The alignment is synthesised on the device (synth.pack_synthetic_device, as bench.py does).  Once: the census and the differing
columns in a handle of their own (tracs_alignment_site_census, tracs_alignment_select_sites), as tracs_distance_tree_bootstrap does.
Then each call runs what the entry point runs per replicate -- the weights over the differing columns, the scan, the new handle, the
gather kernel (tracs_debug_bootstrap_replicate: the library's own functions, the device drained after each), row panels of
tracs_pairsnp_dense_thr without a threshold -> tracs_nj_load_panel, tracs_nj_run, tracs_nj_emit -> tracs_nj_edges ->
tracs_tree_support -- for replicate b = call number, because the entry point takes a FASTA handle and a FASTA of that shape is 50 GB
(scripts/bench_tree.py does the same for the tree).  Reported: per stage the median over the calls, V (the differing columns), the
replicates' lengths, gather's bytes against its time, and everything outside the join loop as a share of the join loop.  For
per-kernel times run it under `rocprofv3 --kernel-trace --stats`, in a run of its own.
--cli: tracs_distance_tree_bootstrap itself, end to end through `python -m tracs_amd distance --tree nj --bootstrap B --tree-edges
--bootstrap-trees` under TRACS_STAGE_TRACE on a lineage-structured FASTA written to a temporary folder.
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


def emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(line + "\n")


def cli(args):
    import hashlib
    import re
    import subprocess

    from tracs_amd import synth
    n, L, B = args.samples, args.sites, args.replicates
    tmp = tempfile.mkdtemp(prefix="tracs_bootstrap_")
    try:
        seqs = synth.alignment(n, L, seed=5, mu_lineage=2e-3, mu_sample=5e-4, n_lineages=20, p_n=0.01)
        fa = os.path.join(tmp, "bench_combined.fasta")
        synth.write_fasta(fa, seqs, names=["sample_%05d" % i for i in range(n)])
        del seqs
        nwk, edges, trees = os.path.join(tmp, "t.nwk"), os.path.join(tmp, "e.csv"), os.path.join(tmp, "b.nwk")
        t0 = time.perf_counter()
        rc = subprocess.run([sys.executable, "-m", "tracs_amd", "distance", "--msa", fa, "--tree", "nj", "-o", nwk, "--tree-edges", edges,
                             "--bootstrap", str(B), "--bootstrap-seed", str(args.seed), "--bootstrap-trees", trees, "--loglevel", "ERROR"],
                            cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, TRACS_STAGE_TRACE="1"))
        dt = time.perf_counter() - t0
        if rc.returncode != 0:
            raise SystemExit(rc.stderr[-3000:])
        stages, notes = {}, []
        for line in rc.stderr.splitlines():
            m = re.match(r"\[stage\] (.*?) ([0-9.]+) s( \(.*\))?$", line)
            if m:
                stages[m.group(1)] = stages.get(m.group(1), 0.0) + float(m.group(2))
            elif line.startswith("[stage] "):
                notes.append(line[8:])
        support = []
        with open(edges) as fh:
            next(fh)
            for row in fh:
                s = row.rsplit(",", 2)[1]
                if s != "NA":
                    support.append(int(s))
        with open(nwk, "rb") as fh:
            digest = hashlib.sha256(fh.read()).hexdigest()
        with open(trees, "rb") as fh:
            trees_digest = hashlib.sha256(fh.read()).hexdigest()
        emit(dict(metric="bootstrap_cli_s", value=dt, unit="s", higher_is_better=False, n=n, L=L, replicates=B, seed=args.seed,
                  stages_s=stages, notes=notes, internal_edges=len(support), support_eq_B=sum(1 for s in support if s == B),
                  support_0=sum(1 for s in support if s == 0), panel_rows=os.environ.get("TRACS_FOREST_PANEL_ROWS"),
                  newick_bytes=os.path.getsize(nwk), edges_bytes=os.path.getsize(edges), trees_bytes=os.path.getsize(trees),
                  newick_sha256=digest, trees_sha256=trees_digest), args.out)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=5000000)
    ap.add_argument("--replicates", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="sparse")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cli", action="store_true")
    args = ap.parse_args()
    if args.cli:
        return cli(args)
    import numpy as np
    import torch

    from bench import synth_kw
    from tracs_amd import _lib, api
    from tracs_amd import device as dev
    from tracs_amd import synth
    from tracs_amd.sites import Sites
    n, L = args.samples, args.sites
    aln = dev.Alignment(n, L)
    synth.pack_synthetic_device(aln, seed=20241022 + 2, **synth_kw(0.0, args.workload))
    torch.cuda.synchronize()
    lib = _lib.load()
    t0 = time.perf_counter()
    _, differs = aln.site_census()
    torch.cuda.synchronize()
    t_census = time.perf_counter() - t0
    t0 = time.perf_counter()
    var, kept = aln.select_sites(keep=differs)
    torch.cuda.synchronize()
    t_select = time.perf_counter() - t0
    V = var.L
    words = Sites(differs, None).c_args()[0]
    u64p = C.POINTER(C.c_uint64)
    panel = max(64, min(n, (1 << 28) // n))
    d = torch.empty((panel, n), dtype=torch.int32, device="cuda")
    nn = torch.empty_like(d)

    def tree_of(a):
        """dense panels + load, join loop, emit + lengths -> seconds[3], edges"""
        t = [time.perf_counter()]
        state = dev.nj_init(n)
        for r0 in range(0, n, panel):
            r1 = min(n, r0 + panel)
            dev.pairsnp_dense(a, d, nn, row_begin=r0, row_end=r1, dist_threshold=2147483647, base_row=r0)
            dev.nj_load_panel(state, n, d, nn, row_begin=r0, row_end=r1, per_site=False, base_row=r0)
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        dev.nj_run(state, n)
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        edges = dev.nj_edges(n, *dev.nj_emit(state, n))
        t.append(time.perf_counter())
        return [b - a for a, b in zip(t[:-1], t[1:])], edges

    main_s, main_edges = tree_of(aln)
    lengths = []

    def call(b):
        sec = (C.c_double * 4)()
        h, n_out = C.c_void_p(), C.c_size_t(0)
        _lib.check(lib.tracs_debug_bootstrap_replicate(var._h, L, words.ctypes.data_as(u64p), args.seed, b, sec, C.byref(h), C.byref(n_out)))
        rep = dev.Alignment.__new__(dev.Alignment)
        rep._L, rep._h, rep.n, rep.L = lib, h, n, int(n_out.value)
        lengths.append(rep.L)
        tree_s, edges = tree_of(rep)
        t0 = time.perf_counter()
        count = api.tree_support(n, main_edges, [edges])
        t_support = time.perf_counter() - t0
        rep.close()
        shared = int((count[main_edges[1] >= n] == 1).sum())
        return list(sec) + tree_s[:2] + [tree_s[2] + t_support], shared

    for k in range(args.warmup):
        call(k)
    lengths.clear()
    runs = [call(args.warmup + k) for k in range(args.steps)]
    stages = np.array([r[0] for r in runs])
    med = np.median(stages, axis=0)
    names = ["weights_s", "scan_s", "new_handle_s", "gather_s", "dense_panels_and_load_s", "join_loop_s", "emit_and_support_s"]
    n_pad = (n + 63) // 64 * 64
    rep_len = float(np.median(lengths))
    # gather reads 5 x 16 bytes per sample and source group with a drawn column (at most every group of the V columns) and writes
    # 5 x 16 bytes per sample and output group
    gather_bytes = 80.0 * n_pad * ((V + 127) // 128) + 80.0 * n * ((rep_len + 127) // 128)
    outside = float(med.sum() - med[5])
    out = dict(metric="bootstrap_replicate_s", value=float(np.median(stages.sum(axis=1))), unit="s", higher_is_better=False, n=n, L=L,
               workload=args.workload, steps=args.steps, warmup=args.warmup, seed=args.seed, differing_columns=int(V),
               replicate_lengths=lengths, census_s=t_census, select_differing_s=t_select,
               main_tree_s=dict(dense_panels_and_load_s=main_s[0], join_loop_s=main_s[1], emit_s=main_s[2]),
               stage_s=[[float(x) for x in row] for row in stages], splits_shared_with_main=[r[1] for r in runs],
               gather_bytes_upper=gather_bytes, gather_gb_per_s=float(gather_bytes / med[3] / 1e9) if med[3] > 0 else None,
               outside_join_loop_s=outside, outside_over_join_loop=float(outside / med[5]) if med[5] > 0 else None,
               estimate_for_replicates=dict(replicates=args.replicates, seconds=float(args.replicates * np.median(stages.sum(axis=1)))))
    out.update({k: float(v) for k, v in zip(names, med)})
    emit(out, args.out)


if __name__ == "__main__":
    main()
