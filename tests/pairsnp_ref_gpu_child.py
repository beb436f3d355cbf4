"""dev.pairsnp_dense on every pair-loop case of tests/golden/pairsnp_ref_golden.npz (the reference's own outputs), in a process of
its own because the kernel switches are read once per process: `python tests/pairsnp_ref_gpu_child.py`, the switches in the
environment (tests/test_gpu_pairsnp_ref.py).  Reads the stored fixture only.  Prints which kernel each alignment ran on:

    USED <alignment> <encoding> <kernel> <site classes: 0 / 1>

Per case, exactly the fixture's d and nn: the whole pass; with dist_threshold, the emitted pairs (every other pair comes back past
the threshold or negative); two files as a row panel / column block; and a row panel that starts at a row > 0, written into a
matrix that holds those rows only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import pairsnp_ref_cases as PC  # noqa: E402
from tracs_amd import device as dev  # noqa: E402

FILL = -7                                                           # no distance, and not a cell past a threshold either: never written


def _upper(n, n0):
    i, j = np.triu_indices(n, 1)
    if n0 is not None:
        keep = (i < n0) & (j >= n0)
        i, j = i[keep], j[keep]
    return i, j


def main():
    meta, arrays = PC.load()
    handles, done = {}, set()
    for case in meta["cases"]:
        key = (case["aln"], case["n0"], case["dist"])
        if key in done:                                             # the same pairs from a differently written file: the FASTA route's business
            continue
        done.add(key)
        seqs = arrays["aln/" + case["aln"]]
        n, L = seqs.shape
        if case["aln"] not in handles:
            aln = dev.Alignment(n, L)
            aln.pack(seqs)
            handles[case["aln"]] = aln
        aln = handles[case["aln"]]
        r, c, d, nn, _ = PC.expected(arrays, case)
        n0, dist, name = case["n0"], case["dist"], case["name"]
        D = torch.full((n, n), FILL, dtype=torch.int32, device="cuda")
        N = torch.full((n, n), FILL, dtype=torch.int32, device="cuda")
        geom = {} if n0 is None else dict(row_begin=0, row_end=n0, col_begin=n0)
        if dist == PC.INT_MAX:
            dev.pairsnp_dense(aln, D, N, **geom)
            i, j = _upper(n, n0)
            assert np.array_equal(i, r) and np.array_equal(j, c), (name, "the fixture lists every pair, in row-major order")
        elif dist >= 0:
            dev.pairsnp_dense(aln, D, N, dist_threshold=dist, **geom)
        else:
            continue                                                # dist < 0 emits nothing: nothing for a dense pass to show
        print("USED %s %s %s %d" % (case["aln"], aln.encoding, aln.kernel, aln.site_classes is not None))
        dh, nh = D.cpu().numpy(), N.cpu().numpy()
        assert np.array_equal(dh[r, c], d), (name, "d", np.nonzero(dh[r, c] != d)[0][:8])
        assert np.array_equal(nh[r, c], nn), (name, "nn", np.nonzero(nh[r, c] != nn)[0][:8])
        if dist != PC.INT_MAX:                                      # every pair the reference did not emit: past the threshold, or negative
            i, j = _upper(n, n0)
            emitted = np.zeros((n, n), bool)
            emitted[r, c] = True
            far = dh[i, j][~emitted[i, j]].astype(np.int64)
            assert ((far > dist) | (far < 0)).all() and not (far == FILL).any(), (name, "pairs beyond the threshold")
        if dist == PC.INT_MAX and n0 is None and n >= 3:
            # a row panel that starts at a row > 0: rows [a, b) into a matrix of b - a rows
            a, b = n // 3, max(n // 3 + 1, (2 * n) // 3)
            P = torch.full((b - a, n), FILL, dtype=torch.int32, device="cuda")
            Q = torch.full((b - a, n), FILL, dtype=torch.int32, device="cuda")
            dev.pairsnp_dense(aln, P, Q, row_begin=a, row_end=b, base_row=a)
            sel = (r >= a) & (r < b)
            assert sel.any()
            assert np.array_equal(P.cpu().numpy()[r[sel] - a, c[sel]], d[sel]), (name, "panel d")
            assert np.array_equal(Q.cpu().numpy()[r[sel] - a, c[sel]], nn[sel]), (name, "panel nn")
    for aln in handles.values():
        aln.close()
    print("DONE %d" % len(done))


if __name__ == "__main__":
    main()
