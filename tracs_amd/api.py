"""Python face of libtracs_hip.so: the four functions of the reference's pybind11 module `TRACS`
(/root/reference/src/python_bindings.cpp:12-25) with the same names, keyword names, return shapes
and error behaviour, plus array-returning variants for callers that do not want Python lists.

All arithmetic runs in HIP kernels (tracs_amd/csrc/*.hip).  No CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from .handle import DistanceHandle, input_paths, require_files, run_arrays


def pairsnp_arrays(fasta, n_threads=1, dist=2147483647, filter=False, sites=None, info=None, max_sample_n_share=None, max_n_share=None,
                   min_sites=None):
    """Like pairsnp() but returns numpy arrays: (rows, cols, distances, names, filt_distances, n_compared).
    sites (tracs_amd.sites.Sites): the run on the files with the dropped columns deleted.  info: a dict that
    receives "seqlen", the alignment length the result stands for (the kept columns).
    max_sample_n_share G: the run on the files without the records that are N at more than floor(G L') of the L' columns
    sites.keep leaves; max_n_share F: columns dropped where more than floor(F n') of the n' surviving samples are N; min_sites M:
    only pairs compared over at least M kept sites.  names, rows and cols are the surviving samples; info then
    also receives "source_names", "n_counts", "kept" (per record read) and "rule_sites" (L')."""
    return _result_arrays(*run_arrays("tracs_pairsnp_rules", input_paths(fasta), None, n_threads, dist, filter, sites, info,
                                      max_sample_n_share, max_n_share, min_sites))


def nearest_arrays(fasta, k, n_threads=1, dist=2147483647, filter=False, sites=None, info=None, max_sample_n_share=None, max_n_share=None,
                   min_sites=None):
    """The k nearest neighbours of each sample (tracs_nearest, include/tracs_hip.h): the six arrays of pairsnp_arrays, rows = the
    sample (ascending), cols = its neighbours ranked by (SNP distance, sample index), at most k per sample.  One file: candidates
    are all other samples; two files: the samples of file 0 get lists, their candidates are the samples of file 1.  Only pairs
    with d <= dist are eligible.  filter: the filtered distances of the emitted pairs (the ranking uses the raw distance).
    n_threads is accepted for parity with pairsnp_arrays and unused: every stage runs on the GPU.  sites, max_sample_n_share,
    max_n_share, min_sites, info: as pairsnp_arrays (the k nearest among the eligible pairs of the surviving samples)."""
    paths = input_paths(fasta, existing=False)
    k = int(k)
    if k < 1 or k > 1024:
        raise ValueError("nearest_arrays(): k must be in [1, 1024], got %d" % k)
    return _result_arrays(*run_arrays("tracs_nearest_rules", require_files(paths), k, n_threads, dist, filter, sites, info,
                                      max_sample_n_share, max_n_share, min_sites))


def group_labels(names, groups):
    """int32 label per sample name for tracs_distance_histogram: groups maps name -> label (any hashable; missing or None:
    ungrouped = -1); labels are numbered in order of first appearance.  None -> None."""
    if groups is None:
        return None
    number = {}
    out = np.full(len(names), -1, np.int32)
    for i, name in enumerate(names):
        lab = groups.get(name)
        if lab is not None:
            out[i] = number.setdefault(lab, len(number))
    return out


def read_histogram_rows(path):
    """The rows of a `distance --histogram` file (header skipped) -> {column: {ref: (value, within, between, ungrouped)}}, numpy
    arrays (uint32; uint64) in file order."""
    got = {}
    with open(path, "r") as fh:
        next(fh, None)
        for ln, line in enumerate(fh, 2):
            f = line.rstrip("\n").split(",", 5)
            if len(f) != 6:
                raise ValueError("%s line %d: expected 6 fields (column,distance,within,between,ungrouped,MSA file)" % (path, ln))
            got.setdefault(f[0], {}).setdefault(f[5], []).append((int(f[1]), int(f[2]), int(f[3]), int(f[4])))
    out = {}
    for col, refs in got.items():
        for ref, rows in refs.items():
            a = np.array(rows, dtype=np.uint64).reshape(-1, 4)
            out.setdefault(col, {})[ref] = (a[:, 0].astype(np.uint32), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy())
    return out


def distance_histogram(fasta, dist=2147483647, filter=False, groups=None, sites=None, max_sample_n_share=None, max_n_share=None,
                       min_sites=None, info=None):
    """How many pairs have each SNP distance (tracs_distance_histogram, include/tracs_hip.h): the pairs pairsnp_arrays(fasta, dist=dist)
    returns, counted on the GPU without being emitted.  -> (names, {"snp": h[, "filter": h]}) with h = {"value": uint32[], "within":
    uint64[], "between": uint64[], "ungrouped": uint64[]}, the non-empty bins ascending.  groups: mapping sample name -> label (any
    hashable; missing or None: ungrouped); without it every pair is `ungrouped`.  filter: also the histogram of the filtered
    distances of the same pairs.  sites, max_sample_n_share, max_n_share, min_sites, info: as pairsnp_arrays (names are the
    surviving samples, only eligible pairs are counted)."""
    import tempfile
    with DistanceHandle(fasta, sites, max_sample_n_share, max_n_share, min_sites) as h:
        _handle_info(h, info, max_sample_n_share is not None or max_n_share is not None or min_sites is not None)
        names = h.names
        labels = group_labels(names, groups)
        gp = labels.ctypes.data_as(C.POINTER(C.c_int32)) if labels is not None and len(labels) else None
        fd, tmp = tempfile.mkstemp(suffix=".csv")
        os.close(fd)
        try:
            with open(tmp, "w") as fh:
                fh.write("header\n")
            eligible, written = C.c_uint64(0), C.c_uint64(0)
            _lib.check(h.L.tracs_distance_histogram(h.h, int(dist), int(bool(filter)), gp, os.fsencode(tmp), b"x", C.byref(eligible),
                                                    C.byref(written)))
            rows = read_histogram_rows(tmp)
        finally:
            os.unlink(tmp)
    empty = (np.zeros(0, np.uint32),) + tuple(np.zeros(0, np.uint64) for _ in range(3))
    out = {}
    for col in ("snp", "filter") if filter else ("snp",):
        v, w, b, u = rows.get(col, {}).get("x", empty)
        out[col] = {"value": v, "within": w, "between": b, "ungrouped": u}
    return names, out


def neighbor_joining(D, method="nj"):
    """The neighbour-joining tree of a symmetric distance matrix (tracs_nj_*), or with method="bionj" its BIONJ tree
    (tracs_bionj_run: the same edges' shape, the reductions weighted by variance): D is a host array or a torch tensor
    (host or device), n x n, finite, non-negative, symmetric with a zero diagonal (else ValueError).  -> parent, child (uint32) and
    length (float64): the 2n - 3 edges in creation order.  Leaves are 0 .. n - 1, join number t makes the node n + t, the last node
    (2n - 3) joins the remaining three; n = 2: the one edge (0, 1, D_01).  Negative lengths are returned as computed."""
    import torch
    from . import device as dev
    if method not in dev.TREE_METHODS:
        raise ValueError("neighbor_joining(): method is 'nj' or 'bionj'")
    _lib.require_gpu()
    M = D if isinstance(D, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(D, dtype=np.float64)))
    if M.dim() != 2 or M.shape[0] != M.shape[1]:
        raise ValueError("neighbor_joining(): D must be a square matrix, got shape %r" % (tuple(M.shape),))
    M = M.to(device="cuda", dtype=torch.float64).contiguous()
    n = int(M.shape[0])
    if n:
        if not bool(torch.isfinite(M).all()):
            raise ValueError("neighbor_joining(): D has a non-finite entry")
        if bool((M < 0).any()):
            raise ValueError("neighbor_joining(): D has a negative entry")
        if bool((torch.diagonal(M) != 0).any()):
            raise ValueError("neighbor_joining(): D has a non-zero diagonal entry")
        if not bool((M == M.t()).all()):
            raise ValueError("neighbor_joining(): D is not symmetric")
    state = dev.nj_init(n, method=method)
    if n >= 2:
        dev.nj_load_f64(state, n, M)
    (dev.bionj_run if method == "bionj" else dev.nj_run)(state, n)
    return dev.nj_edges(n, *dev.nj_emit(state, n))


def tree_support(n, main_edges, replicate_edges):
    """Bootstrap support (tracs_tree_support, host only): main_edges = (parent, child[, length]) of a tree over the
    leaves 0 .. n - 1 as neighbor_joining returns it, replicate_edges = a list of such trees over the same leaves.  -> uint32 per edge
    of the main tree: for an internal edge (its child is an internal node) the number of replicate trees that have an internal edge
    with the same split of the leaves, else 0xFFFFFFFF.  n < 4: no internal edge."""
    L = _lib.load()
    n = int(n)
    parent, child = (np.ascontiguousarray(x, np.uint32) for x in main_edges[:2])
    if parent.shape != child.shape or parent.ndim != 1:
        raise ValueError("tree_support(): parent and child must be two arrays of one length")
    count = np.zeros(len(parent), np.uint32)
    for rep in replicate_edges:
        rp, rc = (np.ascontiguousarray(x, np.uint32) for x in rep[:2])
        if rp.shape != rc.shape or rp.ndim != 1:
            raise ValueError("tree_support(): parent and child must be two arrays of one length")
        _lib.check(L.tracs_tree_support(n, parent.ctypes.data, child.ctypes.data, len(parent), rp.ctypes.data, rc.ctypes.data, len(rp),
                                        count.ctypes.data))
    count[(child < n) | (n < 4)] = 0xFFFFFFFF
    return count


def tree_transfer(n, main_edges, replicate_edges):
    """Transfer bootstrap support (tracs_transfer_*, needs a GPU): main_edges = (parent, child[, length]) of a tree over
    the leaves 0 .. n - 1 as neighbor_joining returns it, replicate_edges = a list of such trees over the same leaves.  -> (sum_phi
    uint64, light uint32, transfer float64), one entry per edge of the main tree: for an internal edge the sum over the replicates of
    the transfer distance phi, the size p of its lighter side, and 1 - sum_phi / (B (p - 1)) in [0, 1]; 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF
    and NaN on leaf edges, and everywhere when n < 4 or there is no replicate."""
    import torch
    L = _lib.require_gpu()
    n = int(n)
    parent, child = (np.ascontiguousarray(x, np.uint32) for x in main_edges[:2])
    if parent.shape != child.shape or parent.ndim != 1:
        raise ValueError("tree_transfer(): parent and child must be two arrays of one length")
    reps = []
    for rep in replicate_edges:
        rp, rc = (np.ascontiguousarray(x, np.uint32) for x in rep[:2])
        if rp.shape != rc.shape or rp.ndim != 1:
            raise ValueError("tree_transfer(): parent and child must be two arrays of one length")
        reps.append((rp, rc))
    sum_phi = np.full(len(parent), 0xFFFFFFFFFFFFFFFF, np.uint64)
    light = np.full(len(parent), 0xFFFFFFFF, np.uint32)
    transfer = np.full(len(parent), np.nan, np.float64)
    if n < 4 or not reps:
        return sum_phi, light, transfer
    nbytes = L.tracs_transfer_state_bytes(n)
    if not nbytes:
        raise ValueError("tree_transfer(): too many leaves")
    state = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.tracs_transfer_init(state.data_ptr(), n, parent.ctypes.data, child.ctypes.data, len(parent), stream))
    for rp, rc in reps:
        _lib.check(L.tracs_transfer_add(state.data_ptr(), n, rp.ctypes.data, rc.ctypes.data, len(rp), None, stream))
    torch.cuda.synchronize()
    _lib.check(L.tracs_transfer_emit(state.data_ptr(), n, sum_phi.ctypes.data, light.ctypes.data))
    inner = child >= n
    den = np.uint64(len(reps)) * (light[inner].astype(np.uint64) - np.uint64(1))
    transfer[inner] = 1.0 - sum_phi[inner].astype(np.float64) / den.astype(np.float64)
    return sum_phi, light, transfer


def pair_sites(fasta, pairs, filter=False, sites=None, info=None, max_sample_n_share=None, max_n_share=None):
    """The SNP sites behind listed pairs -> (offsets int64[m + 1], site uint32[], info uint32[], names): pair t's
    entries are [offsets[t], offsets[t + 1]), ascending by site; site indexes the compared alignment (the kept columns; info receives
    "positions", their columns in the files read); info bits 0-3 / 4-7: the allele masks (A = 1, C = 2, G = 4, T = 8) of the pair's
    first / second sample, bit 8 (filter only): the recombination filter drops the SNP.  pairs: [(a, b), ..], each a sample name or
    an index into names (the surviving samples).  sites, max_sample_n_share, max_n_share, info: as pairsnp_arrays."""
    import torch
    from . import device as dev
    with DistanceHandle(fasta, sites, max_sample_n_share, max_n_share) as h:
        _handle_info(h, info, max_sample_n_share is not None or max_n_share is not None)
        names = h.names
        if info is not None:
            info["positions"] = h.kept_positions()
        index = {}
        for i, name in enumerate(names):
            index[name] = -1 if name in index else i

        def resolve(x):
            if isinstance(x, str):
                if index.get(x, None) is None:
                    raise ValueError("pair_sites(): sample '%s' is not among the samples of the run" % x)
                if index[x] < 0:
                    raise ValueError("pair_sites(): the name '%s' is carried by two samples" % x)
                return index[x]
            if not (0 <= int(x) < len(names)):
                raise ValueError("pair_sites(): sample index %d is outside [0, %d)" % (int(x), len(names)))
            return int(x)
        idx = np.array([(resolve(a), resolve(b)) for a, b in pairs], np.int32).reshape(-1, 2)
        aln = h.alignment()                                                 # the handle's alignment: freed with the handle below
        got = dev.pair_sites(aln, torch.from_numpy(np.ascontiguousarray(idx[:, 0])).cuda(),
                             torch.from_numpy(np.ascontiguousarray(idx[:, 1])).cuda(), filter=filter)
        off, site, bits = (t.cpu().numpy() for t in got)
        aln.close()
    return off, site.view(np.uint32), bits.view(np.uint32), names


def _handle_info(h, info, ruled):
    """info (a dict or None) <- what the sample rule saw (with one of the rule keywords), then "seqlen" (the kept columns)"""
    if info is not None:
        if ruled:
            info.update(h.source())
        info["seqlen"] = int(h.length)


def _result_arrays(L, h):
    """(rows, cols, distances, names, filt_distances, n_compared) of a tracs_pairsnp_result, which they then own."""
    owner = _ResultOwner(L, h)
    n = L.tracs_pairsnp_len(h)
    nseq = L.tracs_pairsnp_nseq(h)

    def grab(fn):
        # a VIEW of the library's result (five arrays of 8 bytes per emitted pair: copying them was a second of a 10 000-sample
        # run); the result handle lives as long as any of the views does
        if n == 0:
            return np.zeros(0, np.uint64)
        v = np.ctypeslib.as_array(fn(h), shape=(n,)).view(_OwnedArray)
        v._tracs_owner = owner
        return v
    rows = grab(L.tracs_pairsnp_rows)
    cols = grab(L.tracs_pairsnp_cols)
    d = grab(L.tracs_pairsnp_distances)
    filt = grab(L.tracs_pairsnp_filt_distances)
    nn = grab(L.tracs_pairsnp_ncompared)
    names = [L.tracs_pairsnp_name(h, i).decode("utf-8", "replace") for i in range(nseq)]
    return rows, cols, d, names, filt, nn


class _ResultOwner:
    """Frees a tracs_pairsnp_result when the last array that views it is gone."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle

    def __del__(self):
        try:
            if self._h:
                self._lib.tracs_pairsnp_free(self._h)
                self._h = None
        except Exception:
            pass


class _OwnedArray(np.ndarray):
    """ndarray view that keeps its owner alive (views and slices of it inherit the reference through `base`)."""
    _tracs_owner = None

    def __array_finalize__(self, obj):
        if obj is not None and getattr(obj, "_tracs_owner", None) is not None:
            self._tracs_owner = obj._tracs_owner


def pairsnp(fasta, n_threads, dist, filter):
    """pairsnp(fasta, n_threads, dist, filter) -> (rows, cols, distances, seq_names, filt_distances,
    n_compared_sites), six Python lists, row-major.  src/python_bindings.cpp:12-13."""
    r, c, d, names, f, nn = pairsnp_arrays(fasta, n_threads, dist, filter)
    return (r.tolist(), c.tolist(), d.tolist(), names, f.tolist(), nn.tolist())


def trans_dist_arrays(snpdiff, datediff, lamb, beta, threshold_Ek):
    n = np.ascontiguousarray(snpdiff, dtype=np.int32)
    d = np.ascontiguousarray(datediff, dtype=np.float64)
    if n.ndim != 1 or d.ndim != 1 or n.shape != d.shape:
        raise ValueError("trans_dist(): snpdiff and datediff must be 1-D and of equal length")
    p0 = np.empty(n.shape[0], np.float64)
    eK = np.empty(n.shape[0], np.float64)
    if n.shape[0]:
        L = _lib.require_gpu()
        _lib.check(L.tracs_trans_dist(n.ctypes.data_as(C.POINTER(C.c_int32)), d.ctypes.data_as(C.POINTER(C.c_double)),
                                      n.shape[0], float(lamb), float(beta), float(threshold_Ek),
                                      p0.ctypes.data_as(C.POINTER(C.c_double)), eK.ctypes.data_as(C.POINTER(C.c_double))))
    return p0, eK


def trans_dist(snpdiff, datediff, lamb, beta, threshold_Ek):
    """trans_dist(snpdiff, datediff, lamb, beta, threshold_Ek) -> (p0_log: list, eK: list).
    src/python_bindings.cpp:19-21 -> src/transcluster.hpp:240-287 (note the order: p0 first)."""
    p0, eK = trans_dist_arrays(snpdiff, datediff, lamb, beta, threshold_Ek)
    return (p0.tolist(), eK.tolist())


def lprob_k_given_N(N, k, delta, lamb, beta, lgamma):
    """lprob_k_given_N(N, k, delta, lamb, beta, lgamma) -> (lprob, lhs).  src/python_bindings.cpp:15-17."""
    if int(N) < 0 or int(k) < 0:
        raise TypeError("lprob_k_given_N(): N and k are unsigned (size_t)")
    lg = np.ascontiguousarray(lgamma, dtype=np.float64)
    Ns = np.array([int(N)], np.uint64)
    ks = np.array([int(k)], np.uint64)
    ds = np.array([float(delta)], np.float64)
    out = np.empty(1), np.empty(1)
    L = _lib.require_gpu()
    u64p, dp = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    _lib.check(L.tracs_lprob_k_given_N(Ns.ctypes.data_as(u64p), ks.ctypes.data_as(u64p), ds.ctypes.data_as(dp), 1,
                                       float(lamb), float(beta), lg.ctypes.data_as(dp), lg.shape[0],
                                       out[0].ctypes.data_as(dp), out[1].ctypes.data_as(dp)))
    return (float(out[0][0]), float(out[1][0]))


def calculate_posteriors(counts, alphas, keep, threshold):
    """calculate_posteriors(counts[L,K], alphas[K], keep, threshold) -> float64[L,K].
    src/python_bindings.cpp:23-25 -> src/dmultinomial.hpp:8-86."""
    c = np.ascontiguousarray(counts, dtype=np.float64)      # py::array_t<double> casts silently
    if c.ndim != 2:
        raise ValueError("calculate_posteriors(): counts must be 2-D [sites, alleles]")
    a = np.ascontiguousarray(alphas, dtype=np.float64)
    if a.ndim != 1 or a.shape[0] != c.shape[1]:
        raise ValueError("calculate_posteriors(): len(alphas) must equal counts.shape[1]")
    out = np.empty_like(c)
    if c.shape[0]:
        L = _lib.require_gpu()
        dp = C.POINTER(C.c_double)
        _lib.check(L.tracs_calculate_posteriors(c.ctypes.data_as(dp), c.shape[0], c.shape[1], a.ctypes.data_as(dp),
                                                int(bool(keep)), float(threshold), out.ctypes.data_as(dp)))
    return out


def connected_components(n_nodes, I, J):
    """Labels of scipy.sparse.csgraph.connected_components(directed=False) (tracs/cluster.py:126-129)."""
    i = np.ascontiguousarray(I, dtype=np.int32)
    j = np.ascontiguousarray(J, dtype=np.int32)
    labels = np.empty(int(n_nodes), np.int32)
    ncomp = C.c_int32(0)
    if n_nodes:
        L = _lib.require_gpu()
        ip = C.POINTER(C.c_int32)
        _lib.check(L.tracs_connected_components(i.ctypes.data_as(ip), j.ctypes.data_as(ip), i.shape[0], int(n_nodes),
                                                labels.ctypes.data_as(ip), C.byref(ncomp)))
    return int(ncomp.value), labels
