#!/usr/bin/env python3
"""The compared alignment's stages on bench.py's workload.  Prints one JSON line and writes it under profiles/msa_out/.

    python scripts/bench_msa_out.py [--samples 10000] [--sites 5000000] [--repeats 5] [--batch-bytes 268435456]

The alignment is synthesised on the device (synth.pack_synthetic_device, as bench.py does).  Three stages, each between HIP events on
the launch stream, one warm-up call and then --repeats timed ones:
    census     site_census_kernel: six counts per site and the differs bitmap (the bitmap stays on the device: no copy in the timing)
    select     tracs_alignment_select_sites under the differs bitmap (the whole call: its list kernels, its host synchronisations, the
               allocation of the new handle -- what --msa-out-sites differing pays; the kernels alone are bench_sites.py's subject)
    unpack     unpack_kernel over one write batch of samples (the rows of --batch-bytes, as tracs_distance_write_alignment cuts them),
               scaled to all samples by the number of batches
Reported are the median and the spread (max - min) of the repeats, the bytes each stage has to move computed from the shapes, the
floor -- those bytes at the 8 TB/s HBM peak -- and the floor's share of the median.
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


def timed(fn, repeats):
    import torch
    fn()                                                    # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=5000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch-bytes", type=int, default=256 << 20)
    ap.add_argument("--out", default=None, help="JSON file (default profiles/msa_out/bench_msa_out_<n>x<L>.json)")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least five")
    import numpy as np
    import torch        # first: one HIP runtime for torch and libtracs_hip

    from bench import synth_kw
    from tracs_amd import _lib, synth
    from tracs_amd import device as dev
    lib = _lib.require_gpu()
    n, L = args.samples, args.sites
    n_pad, groups = (n + 63) // 64 * 64, (L + 127) // 128
    aln = dev.Alignment(n, L)
    synth.pack_synthetic_device(aln, seed=20241022 + 2, **synth_kw(0.0, "sparse"))
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = dict(metric="msa_out_ms", n=n, L=L, repeats=args.repeats, unit="ms", higher_is_better=False)

    counts = torch.empty((6, L), dtype=torch.int32, device="cuda")
    t = timed(lambda: _lib.check(lib.tracs_alignment_site_census(aln._h, C.c_void_p(counts.data_ptr()), None, None, stream)), args.repeats)
    b_census = 4 * 16.0 * n * groups + 6 * 4.0 * L + L / 8.0           # four planes read (N is A & C & G & T), the counts and the bitmap written
    res["census"] = dict(stats(t), bytes=b_census, bytes_five_planes=5 * 16.0 * n_pad * groups + 6 * 4.0 * L)

    _, differs = aln.site_census()
    kept = int(differs.sum())
    res["differing"] = kept
    if kept:
        def select():
            new, _ = aln.select_sites(keep=differs)
            new.close()
        t = timed(select, args.repeats)
        src_groups = int(np.add.reduceat(differs, np.arange(0, L, 128)).astype(bool).sum())
        res["select"] = dict(stats(t), bytes=5 * 16.0 * n_pad * (min(src_groups, kept) + (kept + 127) // 128), note="whole call, host synchronisations included")
    else:
        res["select"] = "not measured (no differing column)"

    stride = (L + 15) // 16 * 16
    batch = max(1, min(n, args.batch_bytes // stride))
    buf = torch.empty((batch, stride), dtype=torch.uint8, device="cuda")
    t = timed(lambda: aln.unpack(first=0, count=batch, stride=stride, out=buf), args.repeats)
    b_unpack = batch * (4 * 16.0 * groups + float(L))
    res["unpack_batch"] = dict(stats(t), bytes=b_unpack, samples=batch)
    scale = n / batch
    res["unpack"] = dict(median_ms=res["unpack_batch"]["median_ms"] * scale, spread_ms=res["unpack_batch"]["spread_ms"] * scale,
                         bytes=b_unpack * scale, note="one batch x n / batch")
    for k in ("census", "select", "unpack_batch", "unpack"):
        if isinstance(res[k], dict):
            floor = res[k]["bytes"] / HBM_PEAK * 1e3
            res[k]["floor_ms"] = floor
            res[k]["floor_share"] = floor / res[k]["median_ms"] if res[k]["median_ms"] > 0 else None
    res["value"] = res["census"]["median_ms"]
    aln.close()
    line = json.dumps(res)
    print(line, flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "msa_out", "bench_msa_out_%dx%d.json" % (n, L))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
