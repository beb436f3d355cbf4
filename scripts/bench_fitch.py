#!/usr/bin/env python3
"""Small parsimony on the neighbour-joining tree of bench.py's workload.  Prints one JSON line; --out FILE also
writes it there.

    python scripts/bench_fitch.py [--samples 10000] [--sites 5000000] [--steps 3] [--warmup 1] [--workload sparse] [--slab-groups G ...]

The alignment is synthesised on the device (synth.pack_synthetic_device, as bench.py does) and its neighbour-joining tree is built
once, as scripts/bench_tree.py builds it.  Then tracs_fitch_count (the leaves kernel, the walk, the offsets scan) and one
tracs_fitch_fill are timed, each as the median of --steps calls after --warmup, the device drained around every call.  The fill covers
the sites from 0 whose entries fit one batch buffer of tracs_distance_tree_changes (256 MiB / 12 bytes), all of them when they fit.
The floor of the count pass is the four allele planes of the leaves read once, n x L / 2 bytes, at the streaming rate DESIGN.md 3.2
records for classify_sites_kernel; `bytes_moved` is what the chosen layout moves on top of that (the leaves written into and read
from the [node][word] buffer twice, the internal sets written, read and overwritten by the states), and `ratio_to_floor` the count
pass's time over the floor.  --slab-groups: one more count pass per given slab length (TRACS_FITCH_SLAB_GROUPS), a single call each.
For per-kernel times run it under `rocprofv3 --kernel-trace --stats`, in a run of its own.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_BYTES_PER_S = 5.97e12          # classify_sites_kernel: 25.12 GB in 4.23 ms (the faster box)
BATCH_ENTRIES = (256 << 20) // 12     # one batch of tracs_distance_tree_changes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=5000000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="sparse")
    ap.add_argument("--slab-groups", type=int, nargs="*", default=[])
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
    for r0 in range(0, n, panel):
        r1 = min(n, r0 + panel)
        dev.pairsnp_dense(aln, d, nn, row_begin=r0, row_end=r1, dist_threshold=2147483647, base_row=r0)
        dev.nj_load_panel(state, n, d, nn, row_begin=r0, row_end=r1, base_row=r0)
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

    os.environ.pop("TRACS_FITCH_SLAB_GROUPS", None)
    for _ in range(args.warmup):
        timed(lambda: dev.fitch_count(aln, parent, child))
    counts = [timed(lambda: dev.fitch_count(aln, parent, child)) for _ in range(args.steps)]
    edge, site, minimum, off, total = counts[-1][1]
    offs = off.cpu().numpy()
    site_end = L if total <= BATCH_ENTRIES else max(int(np.searchsorted(offs, BATCH_ENTRIES, side="right")) - 1, 1)
    entries = int(offs[site_end])
    out3 = tuple(torch.zeros(max(entries, 1), dtype=torch.int32, device="cuda") for _ in range(3))
    fill = lambda: dev.fitch_fill(aln, parent, child, off, 0, site_end, entry_base=0, room=entries, out=out3)      # noqa: E731
    for _ in range(args.warmup):
        timed(fill)
    fills = [timed(fill)[0] for _ in range(args.steps)]
    sweep = {}
    for g in args.slab_groups:
        os.environ["TRACS_FITCH_SLAB_GROUPS"] = str(g)
        sweep[str(g)] = timed(lambda: dev.fitch_count(aln, parent, child))[0]
    os.environ.pop("TRACS_FITCH_SLAB_GROUPS", None)
    count_s = float(np.median([c[0] for c in counts]))
    fill_s = float(np.median(fills))
    changed = (site.cpu().numpy() > 0)
    sum_min = int(minimum.cpu().numpy()[changed].sum())
    nodes = 2 * n - 2 if n >= 3 else n
    floor_bytes = n * L // 2                                               # four planes of the leaves, once
    # per word of 32 sites and 16 bytes per set: the leaves kernel reads and writes n; bottom-up reads 2n - 3 and writes n - 2;
    # top-down reads 2n - 3 sets and n - 2 parents' states and writes n - 3 states
    moved = (L + 31) // 32 * 16 * (2 * n + (2 * n - 3) + (n - 2) + (2 * n - 3) + (n - 2) + (n - 3)) if n >= 3 else floor_bytes
    floor_s = floor_bytes / STREAM_BYTES_PER_S
    out = dict(metric="fitch_count_s", value=count_s, unit="s", higher_is_better=False, n=n, L=L, workload=args.workload, steps=args.steps,
               warmup=args.warmup, count_s=[c[0] for c in counts], fill_s=fill_s, fill_runs_s=fills, fill_sites=site_end, fill_entries=entries,
               tree_build_s=tree_s, parsimony_length=int(total), sum_minimum=sum_min, sites_with_changes=int(changed.sum()),
               consistency_index=(sum_min / total if total else 1.0), edges_with_changes=int((edge.cpu().numpy() != 0).sum()),
               slab_bytes_budget=8 << 30, slab_groups_default=max(1, ((8 << 30) // (nodes * 64)) & ~15), slab_sweep_count_s=sweep,
               floor_bytes=floor_bytes, bytes_moved=moved, stream_bytes_per_s=STREAM_BYTES_PER_S, floor_s=floor_s,
               moved_s_at_stream_rate=moved / STREAM_BYTES_PER_S, ratio_to_floor=count_s / floor_s if floor_s else None,
               ratio_to_moved=count_s / (moved / STREAM_BYTES_PER_S) if moved else None)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
