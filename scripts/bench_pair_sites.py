#!/usr/bin/env python3
"""The passes of `tracs pair-sites` on bench.py's workload.  Prints one JSON line and writes it to
profiles/pair_sites/<workload>_<samples>x<sites>.json.

    python scripts/bench_pair_sites.py [--samples 10000] [--sites 5000000] [--repeats 3] [--pairs 1048576] [--workload sparse]

The alignment is synthesised on the device (synth.pack_synthetic_device, as bench.py does).  Two pair lists:
  forest     the edges of the minimum spanning forest of all pairs by SNP distance (what `distance --mst snp` writes: n - 1 pairs,
             a wave per pair)
  row_major  --pairs seeded pairs i < j in row-major order (a pair per lane)
For each list, from HIP events around the library calls, --repeats times, alternating with the yardstick: the count pass
(tracs_pair_sites_count: count kernel, offsets scan, the total read back), the fill pass (tracs_pair_sites_fill, filter = 0) and fill +
verdicts (filter = 1).  A count or fill pass reads 8 plane rows x L / 8 bytes per pair: bytes / time is the achieved rate.  The
yardstick is tracs_filter_recomb_device on the same list with the distances supplied (the plane scan of `distance --filter` without
departure lists: the same reads, the positions written, the window test reduced to one number per pair); fill + verdicts writes 4
more bytes per SNP and should not be slower beyond the spread of the repeats.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def say(text):
    sys.stderr.write("[bench_pair_sites] %s\n" % text)
    sys.stderr.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=5000000)
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workload", default="sparse")
    ap.add_argument("--max-entries", type=int, default=1 << 31, help="the row-major list is shortened until its entries fit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from bench import synth_kw
    from tracs_amd import _lib
    from tracs_amd import device as dev
    from tracs_amd import synth
    n, L = args.samples, args.sites
    lib = _lib.require_gpu()
    aln = dev.Alignment(n, L)
    synth.pack_synthetic_device(aln, seed=20241022 + 2, **synth_kw(0.0, args.workload))
    torch.cuda.synchronize()
    say("packed %d x %d" % (n, L))

    # the forest's edges, as scripts/bench_forest.py computes them
    panel = max(64, min(n, (1 << 28) // n))
    d = torch.empty((panel, n), dtype=torch.int32, device="cuda")
    nn = torch.empty_like(d)
    state = dev.msf_init(n)
    for r0 in range(0, n, panel):
        r1 = min(n, r0 + panel)
        dev.pairsnp_dense(aln, d, nn, row_begin=r0, row_end=r1, base_row=r0)
        r, c, dd, m = dev.coo_from_dense(d, nn, n, row_begin=r0, row_end=r1, base_row=r0)
        dev.msf_update(state, n, r, c, dd, d=dd, nn=m)
        del r, c, dd, m
    forest = dev.msf_emit(state, n)
    lists = {"forest": (forest[0].contiguous(), forest[1].contiguous())}
    del d, nn, state
    say("forest: %d edges" % lists["forest"][0].numel())
    rng = np.random.default_rng(20241022)
    i = rng.integers(0, n - 1, args.pairs)
    j = i + 1 + (rng.random(args.pairs) * (n - 1 - i)).astype(np.int64)
    order = np.lexsort((j, i))
    lists["row_major"] = (torch.from_numpy(i[order].astype(np.int32)).cuda(), torch.from_numpy(j[order].astype(np.int32)).cuda())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    result = dict(metric="pair_sites_fill_verdict_ms", unit="ms", higher_is_better=False, n=n, L=L, workload=args.workload, repeats=args.repeats,
                  lists={})
    for name, (rows, cols) in lists.items():
        m = int(rows.numel())
        while True:
            dd = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
            off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
            total = C.c_uint64(0)
            _lib.check(lib.tracs_pair_sites_count(aln._h, rows.data_ptr(), cols.data_ptr(), m, dd.data_ptr(), off.data_ptr(), C.byref(total), stream))
            if total.value <= args.max_entries or m <= 1024:
                break
            m //= 2                                                    # (a prefix of a row-major list is row-major)
        k = int(total.value)
        say("%s: %d pairs, %d entries" % (name, m, k))
        site = torch.empty(max(k, 1), dtype=torch.int32, device="cuda")
        info = torch.empty(max(k, 1), dtype=torch.int32, device="cuda")
        pos = torch.empty(max(k, 1), dtype=torch.int32, device="cuda")
        found = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
        filt = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")

        def count():
            _lib.check(lib.tracs_pair_sites_count(aln._h, rows.data_ptr(), cols.data_ptr(), m, dd.data_ptr(), off.data_ptr(), C.byref(total), stream))

        def fill(filter):
            _lib.check(lib.tracs_pair_sites_fill(aln._h, rows.data_ptr(), cols.data_ptr(), m, off.data_ptr(), 0, site.data_ptr(), info.data_ptr(),
                                                 k, filter, stream))

        def yardstick():
            _lib.check(lib.tracs_filter_recomb_device(aln._h, rows.data_ptr(), cols.data_ptr(), m, off.data_ptr(), pos.data_ptr(), found.data_ptr(),
                                                      filt.data_ptr(), stream))
        for fn in (count, lambda: fill(0), lambda: fill(1), yardstick):      # warm-up: code objects, the lgamma table
            fn()
        ms = {"count_ms": [], "fill_ms": [], "fill_verdict_ms": [], "yardstick_ms": []}
        for _ in range(args.repeats):
            ms["yardstick_ms"].append(timed(yardstick))
            ms["fill_verdict_ms"].append(timed(lambda: fill(1)))
            ms["count_ms"].append(timed(count))
            ms["fill_ms"].append(timed(lambda: fill(0)))
        # the two must agree: the kept entries of every pair number the yardstick's filtered distance
        fill(1)
        torch.cuda.synchronize()
        kept = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
        pair_of = torch.repeat_interleave(torch.arange(m, device="cuda"), dd[:m].to(torch.int64))
        kept.index_add_(0, pair_of, ((info[:k] >> 8) == 0).to(torch.int64))
        agree = bool((kept[:m] == filt[:m].to(torch.int64)).all().item()) and bool((found[:m] == dd[:m]).all().item())
        pass_bytes = float(m) * 8.0 * (L / 8.0)
        entry = dict(pairs=m, entries=k, pass_bytes=pass_bytes, agree_with_yardstick=agree)
        for key, v in ms.items():
            best = min(v)
            entry[key] = v
            entry[key.replace("_ms", "_min_ms")] = best
            entry[key.replace("_ms", "_spread_ms")] = max(v) - best
            entry[key.replace("_ms", "_GBps")] = pass_bytes / (best * 1e-3) / 1e9 if best > 0 else None
        entry["verdict_min_ms"] = entry["fill_verdict_min_ms"] - entry["fill_min_ms"]
        entry["fill_verdict_over_yardstick"] = entry["fill_verdict_min_ms"] / entry["yardstick_min_ms"] if entry["yardstick_min_ms"] > 0 else None
        result["lists"][name] = entry
        say("%s done: %s" % (name, json.dumps({k2: entry[k2] for k2 in ("count_min_ms", "fill_min_ms", "fill_verdict_min_ms", "yardstick_min_ms")})))
        del site, info, pos, found, filt, dd, off, kept, pair_of
    result["value"] = result["lists"]["row_major"]["fill_verdict_min_ms"]
    text = json.dumps(result)
    out = args.out or os.path.join(ROOT, "profiles", "pair_sites", "%s_%dx%d.json" % (args.workload, n, L))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    t0 = time.time()
    main()
    say("total %.1f s" % (time.time() - t0))
