#!/usr/bin/env python3
"""`tracs distance --tree nj --tree-edges --tree-changes --tree-sites [--tree-filter --tree-filtered]` end to end, the entry point itself
(DESIGN.md 3.17.1, 3.20, 3.21): wall time, the library's [stage] and [memory] lines under TRACS_STAGE_TRACE, the sizes and hashes of the
files.  Prints one JSON line; --out FILE appends it there.

    python scripts/bench_tree_changes.py --fasta FILE [--filter] [--root CHECKOUT] [--label NAME] [--out FILE]
    python scripts/bench_tree_changes.py --samples 10000 --sites 5000 [--filter]      # a lineage-structured FASTA, written to a temporary folder

--root: the checkout whose `python -m tracs_amd` is run (default: this one) -- two checkouts, one FASTA, one box compare two commits."""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=ROOT)
ap.add_argument("--fasta", default=None)
ap.add_argument("--samples", type=int, default=10000)
ap.add_argument("--sites", type=int, default=5000)
ap.add_argument("--filter", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--label", default=None)
args = ap.parse_args()
tmp = tempfile.mkdtemp(prefix="tracs_changes_")
try:
    if args.fasta is None:
        sys.path.insert(0, ROOT)
        from tracs_amd import synth
        args.fasta = os.path.join(tmp, "bench_combined.fasta")
        synth.write_fasta(args.fasta, synth.alignment(args.samples, args.sites, seed=5, mu_lineage=2e-3, mu_sample=5e-4, n_lineages=20, p_n=0.01),
                          names=["sample_%05d" % i for i in range(args.samples)])
    f = {k: os.path.join(tmp, k) for k in ("t.nwk", "e.csv", "c.csv", "s.csv", "f.nwk")}
    cmd = [sys.executable, "-m", "tracs_amd", "distance", "--msa", args.fasta, "--tree", "nj", "-o", f["t.nwk"], "--tree-edges", f["e.csv"],
           "--tree-changes", f["c.csv"], "--tree-sites", f["s.csv"], "--loglevel", "ERROR"]
    if args.filter:
        cmd += ["--tree-filter", "--tree-filtered", f["f.nwk"]]
    t0 = time.perf_counter()
    rc = subprocess.run(cmd, cwd=args.root, capture_output=True, text=True, env=dict(os.environ, TRACS_STAGE_TRACE="1"))
    dt = time.perf_counter() - t0
    if rc.returncode != 0:
        raise SystemExit(rc.stderr[-3000:])
    stages, memory = {}, {}
    for line in rc.stderr.splitlines():
        m = re.match(r"\[stage\] (.*?) ([0-9.]+) s( \(.*\))?$", line)
        if m:
            stages[m.group(1)] = float(m.group(2))
        m = re.match(r"\[memory\] (.*?) ([0-9.]+) MiB$", line)
        if m:
            memory[m.group(1)] = float(m.group(2))
    files = {k: [os.path.getsize(p), hashlib.sha256(open(p, "rb").read()).hexdigest()[:16]] for k, p in f.items() if os.path.exists(p)}
    out = dict(metric="tree_filter_cli_s" if args.filter else "tree_changes_cli_s", label=args.label, value=dt, unit="s", stages_s=stages,
               memory_mib=memory, files=files)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
finally:
    shutil.rmtree(tmp, ignore_errors=True)
