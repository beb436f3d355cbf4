#!/usr/bin/env python3
"""The branch filter's two device stages on the neighbour-joining tree of bench.py's workload.  Prints one JSON line;
--out FILE also writes it there.

    python scripts/bench_branch_filter.py [--samples 10000] [--sites 5000000] [--steps 3] [--warmup 1] [--workload sparse]

The alignment is synthesised on the device (synth.pack_synthetic_device, as bench.py does) and its neighbour-joining tree is built
once, as scripts/bench_fitch.py builds it.  Then, each as the median of --steps calls after --warmup with the device drained around
every call, in one process on one box:

    tracs_fitch_count          the count pass (what the edge lists start from)
    tracs_fitch_fill           all entries at once: one walk -- the yardstick of the edge-list stage
    tracs_fitch_edge_sites     the changes regrouped by edge: two walks (the chunk matrix, then the placement) and the column scan
    tracs_filter_recomb_lists  the window test on the edges' lists, with the dropped flags
    tracs_fitch_mark_dropped   the verdicts onto the filled entries
    tracs_filter_recomb_pairs  the pair filter on the pairs of the first rows, for its SNPs per second beside the lists' entries per second
                               (the alignment's index is built by the warm-up call and is not in the figure)

`edge_sites_over_fill` is the edge-list stage over one fill (two walks against one); `filter_share` is the lists filter's share of
the device stages of a --tree-filter call (tree, count, edge lists, filter, fill, mark).  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats`, in a run of its own: the four modes of fitch_walk_kernel are separate rows there.
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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="sparse")
    ap.add_argument("--pair-rows", type=int, default=64, help="the pair filter is timed on the pairs (i, j > i) of this many first rows")
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
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    panel = max(64, min(n, (1 << 28) // n))
    d = torch.empty((panel, n), dtype=torch.int32, device="cuda")
    nn = torch.empty_like(d)
    state = dev.nj_init(n)
    pairs = None
    for r0 in range(0, n, panel):
        r1 = min(n, r0 + panel)
        dev.pairsnp_dense(aln, d, nn, row_begin=r0, row_end=r1, dist_threshold=2147483647, base_row=r0)
        dev.nj_load_panel(state, n, d, nn, row_begin=r0, row_end=r1, base_row=r0)
        if r0 == 0:                                                        # the pairs of the first rows, for the pair filter's rate
            k = min(args.pair_rows, r1, n)
            i, j = torch.triu_indices(k, n, offset=1, device="cuda")
            pairs = (i.to(torch.int32).contiguous(), j.to(torch.int32).contiguous(), d[i, j].contiguous())
    dev.nj_run(state, n)
    parent, child, length = dev.nj_edges(n, *dev.nj_emit(state, n))
    del d, nn, state
    torch.cuda.synchronize()
    tree_s = time.perf_counter() - t0

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

    count_s, count_runs, (edge, site, minimum, off, total) = median_of(lambda: dev.fitch_count(aln, parent, child))
    out3 = tuple(torch.zeros(max(total, 1), dtype=torch.int32, device="cuda") for _ in range(3))
    fill_s, fill_runs, (f_site, f_edge, f_info) = median_of(
        lambda: dev.fitch_fill(aln, parent, child, off, 0, L, entry_base=0, room=total, out=out3))
    buf = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
    edge_s, edge_runs, (edge_off, edge_site) = median_of(lambda: dev.fitch_edge_sites(aln, parent, child, edge, room=total, out=buf))
    filt_s, filt_runs, (filt, dropped) = median_of(lambda: dev.filter_recomb_lists(aln, edge_off, edge_site))
    mark_s, mark_runs, _ = median_of(lambda: dev.fitch_mark_dropped(f_site, f_edge, f_info, edge_off, edge_site, dropped))
    pair_s, pair_runs, pair_filt = median_of(lambda: dev.filter_recomb_pairs(aln, *pairs))
    pair_snps = int(pairs[2].to(torch.int64).sum().item())
    # the lists are what the fill says they are: the same (edge, site) multiset, ascending within every edge
    key = f_edge.to(torch.int64) * (L + 1) + f_site.to(torch.int64)
    eo = edge_off.cpu().numpy()
    edge_of = torch.from_numpy(np.repeat(np.arange(len(eo) - 1), np.diff(eo))).cuda()
    same = bool(torch.equal(torch.sort(key).values, edge_of * (L + 1) + edge_site.to(torch.int64)))
    kept = int(filt.to(torch.int64).sum().item())
    changes = edge.cpu().numpy().astype(np.int64)
    stages = tree_s + count_s + edge_s + filt_s + fill_s + mark_s
    out = dict(metric="fitch_edge_sites_s", value=edge_s, unit="s", higher_is_better=False, n=n, L=L, workload=args.workload, steps=args.steps,
               warmup=args.warmup, tree_build_s=tree_s, count_s=count_s, count_runs_s=count_runs, fill_s=fill_s, fill_runs_s=fill_runs,
               edge_sites_s=edge_s, edge_sites_runs_s=edge_runs, edge_sites_over_fill=edge_s / fill_s if fill_s else None,
               one_edge_walk_over_fill=edge_s / 2 / fill_s if fill_s else None,
               filter_lists_s=filt_s, filter_lists_runs_s=filt_runs, entries=int(total), lists=len(eo) - 1,
               longest_list=int(changes.max()) if len(changes) else 0, entries_per_s=total / filt_s if filt_s else None,
               mark_s=mark_s, mark_runs_s=mark_runs, kept=kept, dropped=int(total) - kept,
               edges_with_a_drop=int((filt.cpu().numpy().astype(np.int64) < changes).sum()), lists_equal_the_fill=same,
               pair_filter_s=pair_s, pair_filter_runs_s=pair_runs, pair_filter_pairs=int(pairs[0].numel()), pair_filter_snps=pair_snps,
               pair_filter_snps_per_s=pair_snps / pair_s if pair_s else None, device_stages_s=stages,
               filter_share=filt_s / stages if stages else None, edge_sites_share=edge_s / stages if stages else None,
               matrix_bytes=int((L + 2047) // 2048 * max(len(eo) - 1, 0) * 4), matrix_budget_bytes=256 << 20)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
