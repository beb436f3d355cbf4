"""The allocation path (csrc/alloc_path.h) seen from outside, one case per entry point whose temporaries or structures
became owners: a warm call leaves no block behind, and with every one of its allocations failing in turn the call either raises the
allocation path's message or -- the soft paths: arena, spare blocks, optional lists, filter index -- returns what it returns otherwise,
and in both cases gives back what it took.  Host-side error returns only: nothing here runs the device out of memory.

One alignment serves every case: 70 samples x 300 sites (past SAMPLE_PAD, two site groups and a tail), about 3 % N in runs, a few
partial IUPAC codes; the tree cases take its first 12 samples or a 12-leaf tree.  A case's call opens and closes the handles it uses,
so every round starts from a fresh one.  Two cases run in a child process because their switch is read once per process."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L, N_TREE = 70, 300, 12
MAX_ALLOCS = 40                  # a case that needs more is to be made smaller, not sampled
MESSAGE = re.compile(r"^hip(Host)?Malloc\([^,()]+, \d+ bytes\): \S")


def alignment_text():
    rng = np.random.default_rng(20)
    bases = np.frombuffer(b"ACGT", np.uint8)
    lineage = np.tile(bases[rng.integers(0, 4, size=L)], (5, 1))           # five lineages ~2 % apart, samples ~0.5 % off theirs: the
    for row in lineage:                                                     # departures from a reference stay few, so the filter index is built
        at = rng.random(L) < 0.02
        row[at] = bases[rng.integers(0, 4, size=int(at.sum()))]
    seqs = lineage[rng.integers(0, 5, size=N)].copy()
    mut = rng.random((N, L)) < 0.005
    seqs[mut] = bases[rng.integers(0, 4, size=int(mut.sum()))]
    for s in range(N):                                        # ~3 % N, in runs of 3 .. 9
        left = int(0.03 * L)
        while left > 0:
            k = int(rng.integers(3, 10))
            at = int(rng.integers(0, L - k))
            seqs[s, at:at + k] = ord("N")
            left -= k
    part = rng.random((N, L)) < 0.004
    seqs[part] = np.frombuffer(b"MRWSYK", np.uint8)[rng.integers(0, 6, size=int(part.sum()))]
    return np.ascontiguousarray(seqs)


class Fixture:
    """What the cases share, made once per process: the text, its FASTA files, a 12-leaf tree and a replicate of it."""

    def __init__(self, folder):
        from tracs_amd import api, synth
        self.folder = str(folder)
        self.seqs = alignment_text()
        self.fasta = os.path.join(self.folder, "all.fa")
        self.fasta_tree = os.path.join(self.folder, "tree.fa")
        synth.write_fasta(self.fasta, self.seqs, width=70)
        synth.write_fasta(self.fasta_tree, self.seqs[:N_TREE], width=0)
        rng = np.random.default_rng(21)
        trees = []
        for _ in range(2):
            D = np.triu(rng.integers(1, 40, size=(N_TREE, N_TREE)).astype(np.float64), 1)
            trees.append(api.neighbor_joining(D + D.T)[:2])
        self.tree, self.replicate = trees

    def path(self, name):
        return os.path.join(self.folder, name)


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def packed(fx):
    from tracs_amd import device as dev
    aln = dev.Alignment(N, L)
    try:
        aln.pack(fx.seqs)
    except Exception:
        aln.close()
        raise
    return aln


def dense(aln):
    import torch
    from tracs_amd import device as dev
    dist = torch.zeros((aln.n, aln.n), dtype=torch.int32, device="cuda")
    ncomp = torch.zeros_like(dist)
    dev.pairsnp_dense(aln, dist, ncomp)
    torch.cuda.synchronize()
    iu = np.triu_indices(aln.n, 1)
    return dist.cpu().numpy()[iu], ncomp.cpu().numpy()[iu]


SEEN = {}        # what the last call of a case saw of its route (not part of its result: a soft failure may take another route)


# ---- the cases: each -> a tuple of arrays / bytes / numbers, the same on every call ----------------------------------------------------
def case_trans_dist(fx):
    from tracs_amd import api
    rng = np.random.default_rng(1)
    return api.trans_dist_arrays(rng.integers(0, 40, size=500), rng.random(500) * 2.0, 5.3, 6.0, 0.01)


def case_lprob_k_given_N(fx):
    from math import lgamma
    from tracs_amd import api
    return api.lprob_k_given_N(7, 3, 0.8, 5.3, 6.0, [lgamma(x) if x else 0.0 for x in range(64)])


def case_connected_components(fx):
    from tracs_amd import api
    rng = np.random.default_rng(2)
    k, labels = api.connected_components(200, rng.integers(0, 200, size=150), rng.integers(0, 200, size=150))
    return k, labels


def case_calculate_posteriors(fx):
    from tracs_amd import api
    counts = np.random.default_rng(3).integers(0, 50, size=(300, 4)).astype(np.float64)
    return (api.calculate_posteriors(counts, [0.5, 0.4, 0.3, 0.2], True, 0.01),)


def case_dirichlet_fit(fx):
    from tracs_amd.dirichlet_multinomial import find_dirichlet_priors
    rng = np.random.default_rng(4)
    counts = rng.multinomial(60, [0.9, 0.05, 0.03, 0.02], size=300).astype(np.float64)
    return (find_dirichlet_priors(counts, max_iter=50),)


def case_distance_pair_sites(fx):
    from tracs_amd import _lib
    from tracs_amd.handle import DistanceHandle
    rows = np.arange(0, 20, dtype=np.uint32)
    cols = np.arange(50, 70, dtype=np.uint32)
    out = fx.path("pair_sites.csv")
    u32p = C.POINTER(C.c_uint32)
    with DistanceHandle([fx.fasta]) as h:
        written = C.c_uint64(0)
        _lib.check(h.L.tracs_distance_pair_sites(h.h, rows.ctypes.data_as(u32p), cols.ctypes.data_as(u32p), len(rows), 1, 10 ** 8,
                                                 os.fsencode(out), None, None, 0, 1, C.byref(written)))
    return int(written.value), read(out)


def case_tree_changes_filtered(fx):
    from tracs_amd.handle import DistanceHandle
    names = ["tree.nwk", "edges.csv", "changes.csv", "sites.csv"]
    for name in names:
        if os.path.exists(fx.path(name)):
            os.remove(fx.path(name))
    with DistanceHandle([fx.fasta_tree]) as h:
        res = h.tree(fx.path(names[0]), "ref", edges_path=fx.path(names[1]), changes_path=fx.path(names[2]), sites_path=fx.path(names[3]),
                     tree_filter=True, n_threads=1)
    return (tuple(res),) + tuple(read(fx.path(name)) for name in names)


def case_tree_support_and_transfer(fx):
    from tracs_amd import _lib, api
    lib = _lib.load()
    n_edges = len(fx.tree[0])
    support = api.tree_support(N_TREE, fx.tree, [fx.replicate])                    # host only: no allocation of its own
    phi = np.full(n_edges, 0xFFFFFFFF, np.uint32)
    _lib.check(lib.tracs_tree_transfer(N_TREE, fx.tree[0].ctypes.data, fx.tree[1].ctypes.data, n_edges, fx.replicate[0].ctypes.data,
                                       fx.replicate[1].ctypes.data, len(fx.replicate[0]), phi.ctypes.data))
    return support, phi


def case_gather_sites(fx):
    from tracs_amd import device as dev
    aln = packed(fx)
    new = None
    try:
        new = dev.gather_sites(aln, dev.bootstrap_weights(L, 5, 0))
        return (new.L, new.unpack().cpu().numpy())
    finally:
        if new is not None:
            new.close()
        aln.close()


def case_select_sites(fx):
    aln = packed(fx)
    new = None
    try:
        keep = np.ones(L, bool)
        keep[::7] = False
        new, kept = aln.select_sites(keep=keep, max_n_samples=3)
        return kept, new.unpack().cpu().numpy()
    finally:
        if new is not None:
            new.close()
        aln.close()


def case_sample_n_counts(fx):
    aln = packed(fx)
    try:
        keep = np.ones(L, bool)
        keep[::5] = False
        return (aln.sample_n_counts(keep=keep).cpu().numpy(),)
    finally:
        aln.close()


def case_select_samples(fx):
    aln = packed(fx)
    new = None
    try:
        new = aln.select_samples(np.arange(N) % 3 != 1)
        return (new.n, new.unpack().cpu().numpy())
    finally:
        if new is not None:
            new.close()
        aln.close()


def case_site_census(fx):
    from tracs_amd import _lib
    from tracs_amd.handle import DistanceHandle
    with DistanceHandle([fx.fasta]) as h:
        counts = np.zeros((6, h.length), np.uint32)
        differs = np.zeros((h.length + 63) // 64, np.uint64)
        n_differs = C.c_size_t(0)
        _lib.check(h.L.tracs_distance_site_census(h.h, counts.ctypes.data, differs.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n_differs)))
    return counts, differs, int(n_differs.value)


def case_pack_from_host_text(fx):
    aln = packed(fx)
    try:
        return (aln.unpack().cpu().numpy(),)
    finally:
        aln.close()


def case_dense(fx):
    aln = packed(fx)
    try:
        got = dense(aln)
        SEEN["kernel"] = aln.kernel
        return got
    finally:
        aln.close()


def case_filter_recomb_pairs(fx):
    import torch
    from tracs_amd import device as dev
    aln = packed(fx)
    try:
        d, _ = dense(aln)
        iu = np.triu_indices(N, 1)
        rows, cols = (torch.from_numpy(x.astype(np.int32)).cuda() for x in iu)
        filt = dev.filter_recomb_pairs(aln, rows, cols, torch.from_numpy(d).cuda())
        SEEN["filter_lists"] = dev.filter_index_info(aln)["lists"]
        return d, filt.cpu().numpy()
    finally:
        aln.close()


IN_PROCESS = ["trans_dist", "lprob_k_given_N", "connected_components", "calculate_posteriors", "dirichlet_fit", "distance_pair_sites",
              "tree_changes_filtered", "tree_support_and_transfer", "gather_sites", "select_sites", "sample_n_counts", "select_samples",
              "site_census", "pack_from_host_text", "filter_recomb_pairs"]
# (name, the case it runs, the switch that is read once per process)
IN_CHILD = [("dense_general_mfma", "dense", {"TRACS_GENERAL_MFMA": "1"}),           # gs_build: the general-sparse lists
            ("dense_without_arena", "dense", {"TRACS_PACK_ARENA": "0"})]            # the pack blocks: every pack_alloc is a block of its own


def same(a, b):
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def check_case(name, call, warm_fallback=None):
    """The two checks on one case; prints the figures it asserts on.  warm_fallback: a second warm-up call, for a case whose soft
    failure takes a route with grow-only scratch slots of its own (they stay with the process, as the first route's do)."""
    from tracs_amd import device as dev
    dev.fail_alloc(0)
    if warm_fallback is not None:
        warm_fallback()
    warm = call()                                 # warms the grow-only slots and the process-lifetime tables
    base = dev.alloc_stats()
    again = call()
    after = dev.alloc_stats()
    allocs = after[3]
    print("%s: warm level %d device blocks, %d bytes, %d pinned blocks; a warm call makes %d allocations" % ((name,) + base[:3] + (allocs,)))
    assert after[:3] == base[:3], "a warm call left blocks behind: %r -> %r" % (base, after)
    assert same(again, warm), "two calls, two results"
    assert allocs <= MAX_ALLOCS, "%d allocations: shrink the case" % allocs
    raised = []
    for k in range(1, allocs + 1):
        dev.fail_alloc(k)
        try:
            got = call()
        except RuntimeError as e:
            assert MESSAGE.match(str(e)), "allocation %d of %d: %s" % (k, allocs, e)
            raised.append(k)
        else:
            assert same(got, warm), "allocation %d of %d failed softly and the result changed" % (k, allocs)
        finally:
            dev.fail_alloc(0)
        left = dev.alloc_stats()
        assert all(x <= y for x, y in zip(left[:3], base[:3])), "allocation %d of %d failing left blocks behind: %r -> %r" % (k, allocs, base, left)
    print("%s: %d of %d failures raised, %d were absorbed" % (name, len(raised), allocs, allocs - len(raised)))
    final = call()
    assert same(final, warm), "after the failures the call returns something else"
    assert dev.alloc_stats()[:3] == base[:3]
    return allocs


@pytest.fixture(scope="module")
def fx(hiplib, tmp_path_factory):
    import torch                     # first: one HIP runtime for torch and the library  # noqa: F401
    return Fixture(tmp_path_factory.mktemp("alloc"))


@pytest.mark.parametrize("name", IN_PROCESS)
def test_no_block_left_behind_and_every_allocation_failing_in_turn(fx, name):
    call = lambda: globals()["case_" + name](fx)               # noqa: E731
    if name != "filter_recomb_pairs":
        assert check_case(name, call) >= 1
        return

    def scan_route():
        # without its lists (a failed allocation of the index ends there too) the filter scans the planes, through four scratch
        # slots the list route never asks for; TRACS_FILTER_LISTS is read on every call
        os.environ["TRACS_FILTER_LISTS"] = "0"
        try:
            call()
            assert not SEEN["filter_lists"]
        finally:
            del os.environ["TRACS_FILTER_LISTS"]
    assert check_case(name, call, warm_fallback=scan_route) >= 1
    assert SEEN["filter_lists"], "the filter index was not built: the case does not reach it"


def test_tree_support_allocates_nothing(fx):
    from tracs_amd import api, device as dev
    dev.alloc_stats()
    api.tree_support(N_TREE, fx.tree, [fx.replicate])
    assert dev.alloc_stats()[3] == 0


@pytest.mark.parametrize("name, case, env", IN_CHILD, ids=[c[0] for c in IN_CHILD])
def test_in_a_child_process(hiplib, tmp_path, name, case, env):
    child_env = dict(os.environ)
    for key in ("TRACS_GENERAL_MFMA", "TRACS_PACK_ARENA", "TRACS_FORCE_GENERAL", "TRACS_LIST_CAP"):
        child_env.pop(key, None)
    child_env.update(env)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_alloc as T; T.run_child(%r, %r, %r)" % (
        ROOT, os.path.join(ROOT, "tests"), name, case, str(tmp_path))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=child_env, timeout=600, cwd=ROOT)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]


def run_child(name, case, folder):
    import torch                     # noqa: F401
    fx = Fixture(folder)
    allocs = check_case(name, lambda: globals()["case_" + case](fx))
    assert allocs >= 1
    if name == "dense_general_mfma":
        assert SEEN["kernel"] == "mfma-general", "the dense call took the %s kernel: the case does not reach gs_build" % SEEN["kernel"]
