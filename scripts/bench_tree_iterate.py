#!/usr/bin/env python3
"""The stages of `--tree-filter --tree-iterate K` on bench.py's workload, through the device entry points.  Prints one
JSON line; --out FILE also writes it there.

    python scripts/bench_tree_iterate.py [--samples 10000] [--sites 5000000] [--iterations 3] [--steps 3] [--warmup 1] [--workload sparse]

The alignment is synthesised on the device (synth.pack_synthetic_device, as bench.py does).  Then K iterations of the loop that
tracs_distance_tree_iterate runs, each stage timed with the device drained around it:

    clone / restore            tracs_alignment_clone (iteration 1), then tracs_alignment_restore: the device-to-device copy of the planes
    mask                       tracs_alignment_mask_subtrees on the clone, with W (the (entry, leaf) cells), the cells newly N, cells / s
    pair call on the clone     the dense panels into the neighbour-joining state (the first call after a mask re-decides the pack)
    NJ                         tracs_nj_run + emit + edges
    count / edge lists / filter  tracs_fitch_count, tracs_fitch_edge_sites, tracs_filter_recomb_lists on the ORIGINAL alignment

and, on the first tree's verdicts, restore + mask as the median of --steps calls after --warmup beside the median of
tracs_fitch_count in the same process: the yardstick is `mask_and_restore_over_count` <= 1.  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats`, in a run of its own.

The stage times are whole calls (`mask_s` includes the host's offset check and the call's three stream synchronisations, so cells / s
is the call's rate, not the atomics').  The script is one process and sets no time limit of its own: start it, and the run under the
profiler, each under a `timeout` sized to it (`timeout -k 10 400 python scripts/bench_tree_iterate.py ...`).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=5000000)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="sparse")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from bench import synth_kw
    from tracs_amd import device as dev
    from tracs_amd import synth
    n, L = args.samples, args.sites
    aln = dev.Alignment(n, L)
    synth.pack_synthetic_device(aln, seed=20241022 + 2, **synth_kw(0.0, args.workload))

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        got = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t, got

    def median_of(f):
        for _ in range(args.warmup):
            timed(f)
        runs = [timed(f) for _ in range(args.steps)]
        return float(np.median([r[0] for r in runs])), [r[0] for r in runs], runs[-1][1]

    panel = max(64, min(n, (1 << 28) // n))
    d = torch.empty((panel, n), dtype=torch.int32, device="cuda")
    nn = torch.empty_like(d)

    def tree_of(a):
        state = dev.nj_init(n)

        def panels():
            for r0 in range(0, n, panel):
                r1 = min(n, r0 + panel)
                dev.pairsnp_dense(a, d, nn, row_begin=r0, row_end=r1, dist_threshold=2147483647, base_row=r0)
                dev.nj_load_panel(state, n, d, nn, row_begin=r0, row_end=r1, base_row=r0)

        def joins():
            dev.nj_run(state, n)
            return dev.nj_edges(n, *dev.nj_emit(state, n))
        pair_s, _ = timed(panels)
        nj_s, (parent, child, _) = timed(joins)
        return pair_s, nj_s, parent, child

    def splits(parent, child):
        below, out = {}, set()
        full = (1 << n) - 1
        for p, c in zip(parent.tolist(), child.tolist()):
            m = (1 << c) if c < n else below[c]
            below[p] = below.get(p, 0) | m
            if c >= n:
                out.add(m if not (m & 1) else full & ~m)
        return out

    pair_s, nj_s, parent, child = tree_of(aln)
    rows = [dict(iteration=0, pair_s=pair_s, nj_s=nj_s)]
    seen = [splits(parent, child)]
    clone, stop, first = None, False, None
    for k in range(args.iterations + 1):
        row = rows[-1]
        row["count_s"], (edge, _, _, _, total) = timed(lambda: dev.fitch_count(aln, parent, child))
        row["edge_sites_s"], (edge_off, edge_site) = timed(lambda: dev.fitch_edge_sites(aln, parent, child, edge))
        row["filter_s"], (filt, dropped) = timed(lambda: dev.filter_recomb_lists(aln, edge_off, edge_site))
        changes = edge.cpu().numpy().view(np.uint32).astype(np.int64)
        kept = filt.cpu().numpy().view(np.uint32).astype(np.int64)
        size = np.ones(2 * n, np.int64)
        size[n:] = 0
        for p, c in zip(parent.tolist(), child.tolist()):
            size[p] += size[c]
        work = int(((changes - kept) * size[child.astype(np.int64)]).sum())
        row.update(changes=int(total), kept=int(kept.sum()), dropped=int(total - kept.sum()), W=work)
        if first is None:
            first = (parent, child, edge_off, edge_site, dropped)
        if stop or k == args.iterations:
            break
        if clone is None:
            row["clone_s"], clone = timed(lambda: dev.clone_alignment(aln))
        else:
            row["restore_s"], _ = timed(lambda: dev.restore_alignment(clone, aln))
        row["mask_s"], cells = timed(lambda: dev.mask_subtrees(clone, parent, child, edge_off, edge_site, dropped))
        row.update(masked_cells=cells, cells_per_s=work / row["mask_s"] if row["mask_s"] else None)
        pair_s, nj_s, parent, child = tree_of(clone)
        mine = splits(parent, child)
        rows.append(dict(iteration=k + 1, pair_s=pair_s, nj_s=nj_s, shared_splits=len(mine & seen[-1]),
                         same_as=next((j for j, s in enumerate(seen) if s == mine), None)))
        stop = rows[-1]["same_as"] is not None
        seen.append(mine)
    # the yardstick: the restore + the mask of the first tree's verdicts, beside the count pass, medians in this process
    if clone is None:
        clone = dev.clone_alignment(aln)

    def mask_and_restore():
        dev.restore_alignment(clone, aln)
        return dev.mask_subtrees(clone, *first)
    count_s, count_runs, _ = median_of(lambda: dev.fitch_count(aln, first[0], first[1]))
    both_s, both_runs, cells = median_of(mask_and_restore)
    out = dict(metric="tree_iterate_mask_and_restore_s", value=both_s, unit="s", higher_is_better=False, n=n, L=L, workload=args.workload,
               steps=args.steps, warmup=args.warmup, iterations=rows, count_s=count_s, count_runs_s=count_runs, mask_and_restore_s=both_s,
               mask_and_restore_runs_s=both_runs, mask_and_restore_over_count=both_s / count_s if count_s else None,
               masked_cells_first=cells, alignment_bytes=int(aln.nbytes))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
