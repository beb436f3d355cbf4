#!/usr/bin/env python3
"""The transfer support stage on bench.py's workload.  Prints one JSON line; --out FILE also writes it there.

    python scripts/bench_transfer.py [--samples 10000] [--sites 5000000] [--steps 3] [--warmup 1] [--workload sparse]
    python scripts/bench_transfer.py --cli [--samples 10000] [--sites 5000] [--replicates 8]       # the entry points themselves

The alignment, its differing columns, the main tree and each call's replicate tree are made as scripts/bench_bootstrap.py makes them
(replicate b = call number).  Once: the membership matrix (tracs_debug_transfer_init: the host's share -- bitsets and transposition --
and the uploads, timed apart).  Per call, with the device drained after each: the program on the host
(tracs_tree_transfer_program), then tracs_transfer_add, which builds the same program again, uploads it and runs
transfer_phi_kernel; add minus program is the upload and the kernel.  Reported: the median over the calls, beside the parent's
per-replicate figures (profiles/bootstrap/bench_bootstrap_10000x5000000.json) when that file is there.  For the kernel's own time
run it under `rocprofv3 --kernel-trace --stats`, in a run of its own.
--cli: `python -m tracs_amd distance --tree nj --bootstrap B` with and without `--bootstrap-support transfer` under
TRACS_STAGE_TRACE on a lineage-structured FASTA written to a temporary folder: the stages of both runs, and the distribution of the
transfer support over the internal edges whose split count is 0.
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
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
    import numpy as np

    from tracs_amd import synth
    n, L, B = args.samples, args.sites, args.replicates
    tmp = tempfile.mkdtemp(prefix="tracs_transfer_")
    try:
        seqs = synth.alignment(n, L, seed=5, mu_lineage=2e-3, mu_sample=5e-4, n_lineages=20, p_n=0.01)
        fa = os.path.join(tmp, "bench_combined.fasta")
        synth.write_fasta(fa, seqs, names=["sample_%05d" % i for i in range(n)])
        del seqs
        runs = {}
        for kind in ("split", "transfer"):
            nwk, edges, trees = (os.path.join(tmp, kind + ext) for ext in (".nwk", ".csv", ".trees"))
            t0 = time.perf_counter()
            rc = subprocess.run([sys.executable, "-m", "tracs_amd", "distance", "--msa", fa, "--tree", "nj", "-o", nwk, "--tree-edges", edges,
                                 "--bootstrap", str(B), "--bootstrap-seed", str(args.seed), "--bootstrap-trees", trees, "--loglevel", "ERROR"] +
                                (["--bootstrap-support", "transfer"] if kind == "transfer" else []),
                                cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, TRACS_STAGE_TRACE="1"))
            dt = time.perf_counter() - t0
            if rc.returncode != 0:
                raise SystemExit(rc.stderr[-3000:])
            stages, notes = {}, []
            for line in rc.stderr.splitlines():
                m = re.match(r"\[stage\] (.*?) ([0-9.]+) s( \(.*\))?$", line)
                if m:
                    stages[m.group(1)] = stages.get(m.group(1), 0.0) + float(m.group(2))
                    if m.group(3) and "program" in m.group(3):
                        notes.append(line[8:])
                elif line.startswith("[stage] "):
                    notes.append(line[8:])
            runs[kind] = dict(seconds=dt, stages_s=stages, notes=notes, files=(nwk, edges, trees))
        support, transfer = [], []
        with open(runs["transfer"]["files"][1]) as fh:
            next(fh)
            for row in fh:
                f = row.rstrip("\n").split(",")
                if f[-3] != "NA":
                    support.append(int(f[-3]))
                    transfer.append(float(f[-2]))
        with open(runs["split"]["files"][1]) as fh:
            next(fh)
            split_column = [int(r.rsplit(",", 2)[1]) for r in fh if r.rsplit(",", 2)[1] != "NA"]
        same_trees = open(runs["split"]["files"][2], "rb").read() == open(runs["transfer"]["files"][2], "rb").read()
        support, transfer = np.array(support), np.array(transfer)
        zero = transfer[support == 0]
        q = lambda x: [float(v) for v in np.quantile(x, [0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0])] if len(x) else None      # noqa: E731
        emit(dict(metric="bootstrap_transfer_cli_s", value=runs["transfer"]["seconds"], unit="s", higher_is_better=False, n=n, L=L, replicates=B,
                  seed=args.seed, split_run_s=runs["split"]["seconds"], split_stages_s=runs["split"]["stages_s"],
                  transfer_stages_s=runs["transfer"]["stages_s"], transfer_notes=runs["transfer"]["notes"],
                  internal_edges=int(len(support)), support_column_equal=split_column == support.tolist(), replicate_trees_equal=same_trees,
                  support_eq_B=int((support == B).sum()), support_0=int((support == 0).sum()),
                  transfer_quantiles_0_10_25_50_75_90_100=q(transfer), transfer_of_support_0_quantiles=q(zero),
                  support_0_with_transfer_ge=dict((str(t), int((zero >= t).sum())) for t in (0.5, 0.7, 0.8, 0.9, 0.95, 0.99)),
                  transfer_eq_1=int((transfer == 1.0).sum())), args.out)
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
    from tracs_amd import _lib
    from tracs_amd import device as dev
    from tracs_amd import synth
    from tracs_amd.sites import Sites
    n, L = args.samples, args.sites
    aln = dev.Alignment(n, L)
    synth.pack_synthetic_device(aln, seed=20241022 + 2, **synth_kw(0.0, args.workload))
    torch.cuda.synchronize()
    lib = _lib.load()
    _, differs = aln.site_census()
    var, kept = aln.select_sites(keep=differs)
    torch.cuda.synchronize()
    words = Sites(differs, None).c_args()[0]
    u64p = C.POINTER(C.c_uint64)
    panel = max(64, min(n, (1 << 28) // n))
    d = torch.empty((panel, n), dtype=torch.int32, device="cuda")
    nn = torch.empty_like(d)

    def tree_of(a):
        state = dev.nj_init(n)
        for r0 in range(0, n, panel):
            r1 = min(n, r0 + panel)
            dev.pairsnp_dense(a, d, nn, row_begin=r0, row_end=r1, dist_threshold=2147483647, base_row=r0)
            dev.nj_load_panel(state, n, d, nn, row_begin=r0, row_end=r1, per_site=False, base_row=r0)
        dev.nj_run(state, n)
        torch.cuda.synchronize()
        edges = dev.nj_edges(n, *dev.nj_emit(state, n))
        return tuple(np.ascontiguousarray(x, np.uint32) for x in edges[:2])

    main_p, main_c = tree_of(aln)
    ne = len(main_p)
    state = torch.empty(lib.tracs_transfer_state_bytes(n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    inits = []
    for _ in range(args.warmup + args.steps):
        sec = (C.c_double * 2)()
        t0 = time.perf_counter()
        _lib.check(lib.tracs_debug_transfer_init(state.data_ptr(), n, main_p.ctypes.data, main_c.ctypes.data, ne, sec))
        torch.cuda.synchronize()
        inits.append([sec[0], sec[1], time.perf_counter() - t0])
    inits = np.array(inits[args.warmup:])
    program = np.zeros(2 * n - 3, np.uint32)
    depths = []

    def call(b):
        sec = (C.c_double * 4)()
        h, n_out = C.c_void_p(), C.c_size_t(0)
        _lib.check(lib.tracs_debug_bootstrap_replicate(var._h, L, words.ctypes.data_as(u64p), args.seed, b, sec, C.byref(h), C.byref(n_out)))
        rep = dev.Alignment.__new__(dev.Alignment)
        rep._L, rep._h, rep.n, rep.L = lib, h, n, int(n_out.value)
        rp, rc = tree_of(rep)
        rep.close()
        torch.cuda.synchronize()
        depth = C.c_size_t(0)
        t0 = time.perf_counter()
        _lib.check(lib.tracs_tree_transfer_program(n, rp.ctypes.data, rc.ctypes.data, len(rp), program.ctypes.data, C.byref(depth)))
        t1 = time.perf_counter()
        _lib.check(lib.tracs_transfer_add(state.data_ptr(), n, rp.ctypes.data, rc.ctypes.data, len(rp), None, None))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        depths.append(int(depth.value))
        return [t1 - t0, t2 - t1, (t2 - t1) - (t1 - t0)]

    for k in range(args.warmup):
        call(k)
    _lib.check(lib.tracs_transfer_init(state.data_ptr(), n, main_p.ctypes.data, main_c.ctypes.data, ne, None))      # the sums of the timed calls only
    depths.clear()
    runs = np.array([call(args.warmup + k) for k in range(args.steps)])
    med = np.median(runs, axis=0)
    sums, light = np.zeros(ne, np.uint64), np.zeros(ne, np.uint32)
    _lib.check(lib.tracs_transfer_emit(state.data_ptr(), n, sums.ctypes.data, light.ctypes.data))
    inner = main_c >= n
    x = 1.0 - sums[inner].astype(np.float64) / (float(args.steps) * (light[inner].astype(np.float64) - 1.0))
    out = dict(metric="transfer_stage_s", value=float(med[1]), unit="s", higher_is_better=False, n=n, L=L, workload=args.workload,
               steps=args.steps, warmup=args.warmup, seed=args.seed, internal_edges=int(inner.sum()), waves=int((n - 3 + 63) // 64),
               program_entries=2 * n - 3, program_depths=depths, state_bytes=int(state.numel()),
               program_s=float(med[0]), add_s=float(med[1]), upload_and_kernel_s=float(med[2]), calls_s=[[float(v) for v in r] for r in runs],
               membership_host_s=float(np.median(inits[:, 0])), membership_upload_s=float(np.median(inits[:, 1])),
               membership_s=float(np.median(inits[:, 2])), membership_runs_s=[[float(v) for v in r] for r in inits],
               transfer_quantiles_0_25_50_75_100=[float(v) for v in np.quantile(x, [0, 0.25, 0.5, 0.75, 1.0])])
    parent = os.path.join(ROOT, "profiles", "bootstrap", "bench_bootstrap_10000x5000000.json")
    if os.path.exists(parent) and (n, L) == (10000, 5000000):
        with open(parent) as fh:
            ref = json.loads(fh.readline())
        out["parent_join_loop_s"] = ref.get("join_loop_s")
        out["parent_outside_join_loop_s"] = ref.get("outside_join_loop_s")
        if ref.get("outside_join_loop_s"):
            out["transfer_over_parent_outside_join_loop"] = float(med[1] / ref["outside_join_loop_s"])
    emit(out, args.out)


if __name__ == "__main__":
    main()
