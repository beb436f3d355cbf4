#!/usr/bin/env python3
"""Site rules on bench.py's workload.  Prints one JSON line per selection.

    python scripts/bench_sites.py [--samples 10000] [--sites 5000000] [--repeats 5] [--only NAME]
    python scripts/bench_sites.py --open --samples 2000 --sites 500000      # tracs_distance_open against tracs_distance_open_sites

The alignment is synthesised on the device (synth.pack_synthetic_device, as bench.py does; the coverage-shaped "runs" workload for
the N rule).  Four selections:
    runs5      twenty runs that drop 5 % of the columns
    n_rule     --max-n-share 0.2 on coverage-shaped input
    iid1       1 % of the columns dropped independently (every 32-site word has gaps)
    sparse200  one column in 200 kept
For each, tracs_debug_site_select_timing runs the stages between HIP events -- the N count, the list (bitmap, offsets, list), the
compaction by select_sites_kernel and, on the same list, by the re-pack kernel of the site classes (compact_sites_kernel<0>, what
the parent commit had) -- in alternation, --repeats times after one warm-up round; reported are the median and the spread
(max - min) of the repeats, the bytes each stage moves computed from the shapes, and their share of the 8 TB/s HBM peak.
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def selections(L, n, rng):
    import numpy as np
    runs = np.ones(L, bool)
    run_len = L // 400                                     # twenty runs x L / 400 = 5 %
    for s in rng.choice(L // run_len, 20, replace=False):
        runs[s * run_len:(s + 1) * run_len] = False
    sparse = np.zeros(L, bool)
    sparse[::200] = True
    return [("runs5", "sparse", runs, None), ("n_rule", "runs", None, int(0.2 * n)), ("iid1", "sparse", rng.random(L) >= 0.01, None),
            ("sparse200", "sparse", sparse, None)]


def stats(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "spread_ms": v[-1] - v[0]}


def kernels(args):
    import numpy as np
    import torch

    from bench import synth_kw
    from tracs_amd import _lib, synth
    from tracs_amd import device as dev
    from tracs_amd.sites import bitmap_to_bool, bool_to_bitmap
    lib = _lib.require_gpu()
    n, L = args.samples, args.sites
    aln = dev.Alignment(n, L)
    n_pad, groups = (n + 63) // 64 * 64, (L + 127) // 128
    packed = None
    u64p = C.POINTER(C.c_uint64)
    for name, workload, keep, max_n in selections(L, n, np.random.default_rng(7)):
        if args.only and name != args.only:
            continue
        if packed != workload:
            synth.pack_synthetic_device(aln, seed=20241022 + 2, **synth_kw(0.0, workload))
            torch.cuda.synchronize()
            packed = workload
        words = bool_to_bitmap(keep) if keep is not None else None
        ms = (C.c_float * (4 * args.repeats))()
        n_kept, same = C.c_size_t(0), C.c_int(-1)
        _lib.check(lib.tracs_debug_site_select_timing(aln._h, words.ctypes.data_as(u64p) if words is not None else None, L,
                                                      0xFFFFFFFF if max_n is None else max_n, args.repeats, ms, C.byref(n_kept), C.byref(same)))
        t = np.array(list(ms), np.float64).reshape(args.repeats, 4)
        kept = int(n_kept.value)
        if keep is not None:
            src_groups = int(np.add.reduceat(keep, np.arange(0, L, 128)).astype(bool).sum())
        else:
            # (the N rule's kept columns are only known on the device: the selected handle's bitmap)
            new, kb = aln.select_sites(max_n_samples=max_n)
            new.close()
            src_groups = int(np.add.reduceat(kb, np.arange(0, L, 128)).astype(bool).sum())
        dst_groups = (kept + 127) // 128
        # the kernel's choice, per output group: gather where the group's kept sites span more source groups than it has sites
        idx = np.flatnonzero(kb if keep is None else keep)
        first, last = idx[::128], idx[np.minimum(np.arange(127, kept + 127, 128), kept - 1)]
        gather_groups = int(((last >> 7) - (first >> 7) + 1 > np.minimum(128, kept - np.arange(0, kept, 128))).sum())
        gather = gather_groups * 2 > dst_groups
        b_count = n_pad * groups * 16.0 + 4.0 * L if max_n is not None else 0.0
        b_list = 4.0 * L + 3 * 4.0 * groups * 4 + 4.0 * kept
        # gather reads one dword per kept site, sample and plane, but whole 64-byte sectors move: 16 bytes per lane at best
        b_sel = 5 * 16.0 * n_pad * ((kept if gather else src_groups) + dst_groups)
        out = dict(metric="site_select_ms", selection=name, workload=workload, n=n, L=L, kept=kept, max_n_samples=max_n, repeats=args.repeats,
                   route="gather" if gather else "stream", gather_groups=gather_groups, output_groups=dst_groups, same_bytes_as_compact_kernel=bool(same.value),
                   count=dict(stats(t[:, 0]), bytes=b_count), list=dict(stats(t[:, 1]), bytes=b_list),
                   select=dict(stats(t[:, 2]), bytes=b_sel), compact_kernel=dict(stats(t[:, 3]), bytes=b_sel), unit="ms", higher_is_better=False)
        for k in ("count", "select", "compact_kernel"):
            m = out[k]["median_ms"]
            out[k]["hbm_peak_share"] = (out[k]["bytes"] / (m * 1e-3) / HBM_PEAK) if m > 0 else None
        out["value"] = out["select"]["median_ms"]
        out["select_over_compact_kernel"] = out["select"]["median_ms"] / out["compact_kernel"]["median_ms"]
        print(json.dumps(out), flush=True)
    aln.close()


def opens(args):
    """tracs_distance_open against tracs_distance_open_sites (selection runs5) on a FASTA written to a temporary folder"""
    import shutil
    import tempfile

    import numpy as np

    from tracs_amd import _lib, synth
    from tracs_amd.sites import bool_to_bitmap
    lib = _lib.require_gpu()
    n, L = args.samples, args.sites
    tmp = tempfile.mkdtemp(prefix="tracs_sites_")
    try:
        seqs = synth.alignment(n, L, seed=5, mu_lineage=2e-4, mu_sample=2e-5, n_lineages=20, p_n=0.01)
        fa = os.path.join(tmp, "bench_combined.fasta")
        synth.write_fasta(fa, seqs)
        del seqs
        keep = selections(L, n, np.random.default_rng(7))[0][2]
        words = bool_to_bitmap(keep)
        arr = (C.c_char_p * 1)(os.fsencode(fa))
        plain, ruled = [], []
        for r in range(args.repeats + 1):                   # (round 0: warm-up -- the runtime, the page cache)
            for which in (0, 1):
                h = C.c_void_p()
                t0 = time.perf_counter()
                if which == 0:
                    _lib.check(lib.tracs_distance_open(arr, 1, C.byref(h)))
                else:
                    _lib.check(lib.tracs_distance_open_sites(arr, 1, words.ctypes.data_as(C.POINTER(C.c_uint64)), L, 0xFFFFFFFF, C.byref(h)))
                dt = (time.perf_counter() - t0) * 1e3
                lib.tracs_distance_free(h)
                if r:
                    (plain, ruled)[which].append(dt)
        print(json.dumps(dict(metric="distance_open_sites_ms", n=n, L=L, selection="runs5", kept=int(keep.sum()), repeats=args.repeats,
                              open=stats(plain), open_sites=stats(ruled), value=stats(ruled)["median_ms"], unit="ms", higher_is_better=False)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=5000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--open", action="store_true")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least five")
    import torch        # first: one HIP runtime for torch and libtracs_hip  # noqa: F401
    return opens(args) if args.open else kernels(args)


if __name__ == "__main__":
    main()
