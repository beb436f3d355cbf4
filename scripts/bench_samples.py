#!/usr/bin/env python3
"""The sample rule and the pair rule on bench.py's workload.  Prints one JSON line per stage.

    python scripts/bench_samples.py [--samples 10000] [--sites 5000000] [--drop 0.05] [--repeats 5]

The alignment is synthesised on the device (synth.pack_synthetic_device, as bench.py does).  Three stages between HIP events, one
warm-up round, then --repeats rounds; reported are the median and the spread (max - min) of the repeats, the bytes each stage moves
computed from the shapes, the floor those bytes take at the 8 TB/s HBM peak, and the share of that peak reached:
    count    sample_n_count_kernel under a bitmap that drops 5 % of the columns: plane 4 once, n_pad x groups x 16 bytes
    gather   select_samples_kernel for a mask that drops --drop of the samples: 5 x 16 bytes per kept sample and group, read + written
    veto     pair_min_sites_kernel over one panel of rows x n cells of the upper triangle: 8 bytes read per cell
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def stats(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "spread_ms": v[-1] - v[0]}


def report(metric, times, nbytes, **extra):
    out = dict(metric=metric, **extra, **stats(times), bytes=nbytes, floor_ms=nbytes / HBM_PEAK * 1e3, bound="HBM bandwidth", unit="ms",
               higher_is_better=False)
    out["hbm_peak_share"] = out["floor_ms"] / out["median_ms"] if out["median_ms"] > 0 else None
    out["value"] = out["median_ms"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=5000000)
    ap.add_argument("--drop", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least five")
    import numpy as np
    import torch        # first: one HIP runtime for torch and libtracs_hip

    from bench import synth_kw
    from tracs_amd import _lib, synth
    from tracs_amd import device as dev
    from tracs_amd.sites import bool_to_bitmap
    lib = _lib.require_gpu()
    n, L = args.samples, args.sites
    n_pad, groups = (n + 63) // 64 * 64, (L + 127) // 128
    aln = dev.Alignment(n, L)
    synth.pack_synthetic_device(aln, seed=20241022 + 2, **synth_kw(0.0, "sparse"))
    torch.cuda.synchronize()
    rng = np.random.default_rng(7)
    keep = np.ones(L, bool)
    run_len = max(1, L // 400)                             # twenty runs x L / 400 = 5 % of the columns
    for s in rng.choice(L // run_len, 20, replace=False):
        keep[s * run_len:(s + 1) * run_len] = False
    mask = np.ones(n, np.uint8)
    mask[rng.choice(n, max(1, int(round(args.drop * n))), replace=False)] = 0
    words = bool_to_bitmap(keep)
    ms = (C.c_float * (2 * args.repeats))()
    n_kept = C.c_size_t(0)
    _lib.check(lib.tracs_debug_sample_select_timing(aln._h, words.ctypes.data_as(C.POINTER(C.c_uint64)), L, mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                    args.repeats, ms, C.byref(n_kept)))
    t = np.array(list(ms), np.float64).reshape(args.repeats, 2)
    kept = int(n_kept.value)
    common = dict(n=n, L=L, repeats=args.repeats)
    report("sample_n_count_ms", t[:, 0].tolist(), n_pad * groups * 16.0 + groups * 16.0 + 4.0 * n, columns_kept=int(keep.sum()), **common)
    report("select_samples_ms", t[:, 1].tolist(), 2 * 5 * 16.0 * kept * groups + 4.0 * kept, samples_kept=kept, **common)
    aln.close()
    # the veto pass on a panel as the FASTA entry points cut it (~2^28 cells): distances and compared-sites counts of the shape's range
    rows = max(64, min(n, (1 << 28) // max(n, 1)))
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    d = torch.randint(0, 200, (rows, n), dtype=torch.int32, device="cuda", generator=g)
    nn = torch.randint(L - L // 10, L + 1, (rows, n), dtype=torch.int32, device="cuda", generator=g)
    cells = sum(max(0, n - (i + 1)) for i in range(rows))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for r in range(-1, args.repeats):
        work = d.clone()                                   # (every round vetoes the same cells)
        ev[0].record()
        dev.pairs_min_sites(work, nn, n, L - L // 20, row_begin=0, row_end=rows, dist_threshold=100)
        ev[1].record()
        ev[1].synchronize()
        if r >= 0:
            times.append(ev[0].elapsed_time(ev[1]))
    vetoed = int((work[:, :] == -1).sum().item())
    report("pair_min_sites_ms", times, 8.0 * cells, panel_rows=rows, cells=cells, vetoed=vetoed, **common)


if __name__ == "__main__":
    main()
