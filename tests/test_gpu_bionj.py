"""BIONJ on the device (tracs_bionj_run: csrc/nj.hip) against the definition restated in numpy (tests/bionj_ref.py):
the join records bit for bit -- the joined nodes as integers, D_ab and the row sums as uint64 views -- and `method="bionj"` through the
whole tree route (the main tree, bootstrap replicates, the Fitch stages, the iterated filter) against the same reference."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bionj_ref
import bootstrap_ref
import fitch_ref
import nj_ref

pytestmark = pytest.mark.gpu

SIZES = [4, 5, 6, 17, 64, 256, 257, 513]       # the first join alone; the 256-thread block edge of rows and commit; two blocks
KINDS = ["noisy", "per-site", "duplicates"]


@functools.lru_cache(maxsize=None)
def matrix(n, kind):
    rng = np.random.default_rng(31 * n + len(kind))
    if kind == "noisy":
        D = bionj_ref.noisy_tree_metric(n, 7 * n + 1) if n >= 3 else np.zeros((n, n))
    elif kind == "per-site":                           # SNP counts over the sites compared: quotients that are not dyadic
        d = np.triu(rng.integers(0, 400, (n, n)), 1)
        nn = np.triu(rng.integers(2500, 3000, (n, n)), 1) + np.tril(np.ones((n, n), np.int64))
        D = d.astype(np.float64) / nn.astype(np.float64)
        D = D + D.T
    else:                                              # every third sample is the one before it again
        D = bionj_ref.noisy_tree_metric(n, 5 * n + 2)
        for k in range(1, n, 3):
            D[k] = D[k - 1]; D[:, k] = D[:, k - 1]
            D[k, k - 1] = D[k - 1, k] = 0.0
        np.fill_diagonal(D, 0.0)
        assert np.array_equal(D, D.T)
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def reference(n, kind):
    return bionj_ref.bionj_records(matrix(n, kind))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def assert_same(got, want, what):
    (a, b, dab, ra, rb), ids, d = got
    (wa, wb, wdab, wra, wrb), wids, wd = want
    assert np.array_equal(a, wa) and np.array_equal(b, wb), (what, np.flatnonzero((a != wa) | (b != wb))[:5])
    for name, x, y in (("D_ab", dab, wdab), ("R_a", ra, wra), ("R_b", rb, wrb)):
        assert np.array_equal(bits(x), bits(y)), (what, name, np.flatnonzero(bits(x) != bits(y))[:5])
    assert np.array_equal(ids, wids), (what, ids, wids)
    assert np.array_equal(bits(d), bits(wd)), (what, d, wd)


def run_f64(D, pad=0, method="bionj", run=None):
    import torch

    from tracs_amd import device as dev
    n = D.shape[0]
    M = torch.full((n, n + pad), -1.0, dtype=torch.float64)
    M[:, :n] = torch.from_numpy(np.array(D))
    state = dev.nj_init(n, method=method)
    if n >= 2:
        dev.nj_load_f64(state, n, M.cuda())
    (run or (dev.bionj_run if method == "bionj" else dev.nj_run))(state, n)
    return dev.nj_emit(state, n)


def run_panels(d, bounds, pad=0):
    """d: integer n x n; only the cells j > i are handed over (the rest is poisoned), in the row panels bounds[k] .. bounds[k + 1]"""
    import torch

    from tracs_amd import device as dev
    n = d.shape[0]
    state = dev.nj_init(n, method="bionj")
    upper = np.triu(np.ones((n, n), bool), 1)
    for r0, r1 in zip(bounds[:-1], bounds[1:]):
        pd = np.full((r1 - r0, n + pad), 0x7FFFFFF0, np.int64)
        pd[:, :n] = np.where(upper[r0:r1], d[r0:r1], 0x7FFFFFF0)
        td = torch.from_numpy(pd.astype(np.uint32).view(np.int32)).cuda()
        dev.nj_load_panel(state, n, td, None, row_begin=r0, row_end=r1, base_row=r0)
    dev.bionj_run(state, n)
    return dev.nj_emit(state, n)


def retired_slots(n, rec):
    """the device's slot layout replayed from the records -> how many joins retire the last active slot, how many another one, and how
    many find the lower id in the higher slot"""
    slot = {k: k for k in range(n)}
    at = list(range(n))
    last_is, other, swapped = 0, 0, 0
    for t, (a, b) in enumerate(zip(rec[0].tolist(), rec[1].tolist())):
        r = n - t
        keep, ret = sorted((slot[a], slot[b]))
        swapped += slot[a] > slot[b]
        if ret == r - 1:
            last_is += 1
        else:
            other += 1
            at[ret] = at[r - 1]
            slot[at[ret]] = ret
        at[keep] = n + t
        slot[n + t] = keep
    return last_is, other, swapped


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_records_equal_the_definition_bit_for_bit(hiplib, n, kind):
    assert_same(run_f64(matrix(n, kind)), reference(n, kind), (n, kind))


def test_the_cases_retire_the_last_slot_and_others_and_find_a_in_the_higher_slot():
    """(host arithmetic on the references the test above compares with: the cases cover both moves of the commit, and joins whose
    lower id sits in the higher slot -- where ordering by slot instead of by id would show)"""
    for n, kind in ((17, "noisy"), (64, "per-site"), (257, "duplicates")):
        last_is, other, swapped = retired_slots(n, reference(n, kind)[0])
        assert last_is >= 1 and other >= 1 and last_is + other == n - 3, (n, kind, last_is, other)
        assert swapped >= 1, (n, kind)
    assert sum(retired_slots(n, reference(n, k)[0])[2] for n in SIZES for k in KINDS) > 50


@pytest.mark.parametrize("n,kind", [(17, "noisy"), (257, "noisy"), (64, "duplicates")])
def test_panels_in_any_split_and_with_a_wider_leading_dimension(hiplib, n, kind):
    d = matrix(n, kind).astype(np.int64)
    assert np.array_equal(d.astype(np.float64), matrix(n, kind))
    want = reference(n, kind)
    assert_same(run_panels(d, [0, n], pad=7), want, "ld = n + 7")
    assert_same(run_panels(d, [0, n // 3, n]), want, "two panels")
    assert_same(run_panels(d, [0, 1, n // 4, n // 2, n - 2, n], pad=7), want, "five panels")
    assert_same(run_f64(matrix(n, kind), pad=7), want, "f64, ld = n + 7")


def test_scan_with_several_tiles_per_row_and_per_workgroup(hiplib):
    """n = 2 100, the size of neighbour joining's test of the same name: a folded row of the scan is more than one tile and a workgroup
    strides over tiles.  A tree metric comes back with all its splits; lengths to 1e-9 max(D), as on the host (lambda is not dyadic)."""
    from tracs_amd import device as dev
    n = 2100
    D, want = nj_ref.random_tree_metric(n, np.random.default_rng(11))
    rec, ids, d = run_f64(D)
    parent, child, length = dev.nj_edges(n, rec, ids, d)
    got = nj_ref.splits_of(n, parent, child, length)
    assert len(parent) == 2 * n - 3 and set(got) == set(want)
    assert max(abs(got[s] - want[s]) for s in want) <= 1e-9 * D.max()


def test_the_pinned_matrix_gives_two_different_trees(hiplib):
    from tracs_amd import api
    D = bionj_ref.NJ_DIFFERS
    got_nj, got_bio = api.neighbor_joining(D), api.neighbor_joining(D, method="bionj")
    for got, want in ((got_nj, nj_ref.nj(D)), (got_bio, bionj_ref.bionj(D)), (api.neighbor_joining(D, method="nj"), nj_ref.nj(D))):
        assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert set(nj_ref.splits_of(6, *got_nj)) != set(nj_ref.splits_of(6, *got_bio))
    with pytest.raises(ValueError, match="method"):
        api.neighbor_joining(D, method="upgma")


def test_state_handling(hiplib):
    from tracs_amd import device as dev
    for n in (0, 1, 2, 3):
        D = 7.0 * (np.ones((n, n)) - np.eye(n))
        assert_same(run_f64(D), nj_ref.nj_records(D), n)
    state = dev.nj_init(5, method="bionj")
    with pytest.raises(RuntimeError, match="has not been run"):
        dev.nj_emit(state, 5)
    dev.bionj_run(state, 5)
    with pytest.raises(RuntimeError, match="tracs_bionj_run: the state has been run"):
        dev.bionj_run(state, 5)
    with pytest.raises(RuntimeError, match="has been run"):
        dev.nj_run(state, 5)
    with pytest.raises(RuntimeError, match="another vertex count"):
        dev.bionj_run(dev.nj_init(6, method="bionj"), 5)
    # a NULL state and n above 2^24, as neighbour joining's
    assert hiplib.tracs_bionj_run(None, 5, None) == -1 and hiplib.tracs_nj_run(None, 5, None) == -1
    assert hiplib.tracs_bionj_state_bytes(2 ** 24 + 1) == 0 == hiplib.tracs_nj_state_bytes(2 ** 24 + 1)
    with pytest.raises(ValueError, match="2\\^24"):
        dev.nj_init(2 ** 24 + 1, method="bionj")
    fresh = dev.nj_init(5, method="bionj")
    for run in (hiplib.tracs_bionj_run, hiplib.tracs_nj_run):
        assert run(C.c_void_p(fresh.data_ptr()), 2 ** 24 + 1, None) == -1
    # a state of the smaller size is not handed to the BIONJ loop by the wrapper
    with pytest.raises(ValueError, match="smaller than a BIONJ state"):
        dev.bionj_run(dev.nj_init(64), 64)
    # neighbour joining is untouched: on its own state, and on a BIONJ-sized one
    D = matrix(64, "noisy")
    want = nj_ref.nj_records(D)
    assert_same(run_f64(D, method="nj"), want, "nj on its own state")
    assert_same(run_f64(D, method="bionj", run=dev.nj_run), want, "nj on a BIONJ-sized state")
    assert not np.array_equal(bits(want[0][3]), bits(reference(64, "noisy")[0][3]))                  # (and BIONJ differs there)


# ---- the tree route ---------------------------------------------------------------------------------------------------------------

N, L, SEED, B = 40, 2000, 5, 8


@functools.lru_cache(maxsize=None)
def alignment():
    """40 x 2 000, ACGT only (the SNP distance is then the Hamming distance): five lineages of unequal depth, private changes, two
    samples that are copies of others -> (ASCII uint8[n, L], the distances)"""
    rng = np.random.default_rng(404)
    base = rng.integers(0, 4, L)
    depth = np.array([0.002, 0.01, 0.03, 0.06, 0.1])
    lineage = np.where(rng.random((5, L)) < depth[:, None], rng.integers(0, 4, (5, L)), base)
    idx = lineage[np.arange(N) % 5]
    idx = np.where(rng.random((N, L)) < 0.004, rng.integers(0, 4, (N, L)), idx)
    idx[17], idx[33] = idx[2], idx[9]
    seqs = np.frombuffer(b"ACGT", np.uint8)[idx]
    D = bootstrap_ref.snp_matrix(seqs).astype(np.float64)
    assert np.array_equal(D, (idx[:, None, :] != idx[None, :, :]).sum(axis=2)) and D[2, 17] == 0 and D[9, 33] == 0
    seqs.setflags(write=False); D.setflags(write=False)
    return seqs, D


NAMES = ["s%02d" % i for i in range(N)]


@pytest.fixture(scope="module")
def handle(hiplib, tmp_path_factory):
    from tracs_amd import synth
    from tracs_amd.handle import DistanceHandle
    fa = tmp_path_factory.mktemp("bionj") / "x_combined.fasta"
    synth.write_fasta(str(fa), alignment()[0], names=NAMES, width=60)
    with DistanceHandle([str(fa)]) as h:
        yield h


def host_files(hiplib, folder, edges, ref="x"):
    """the Newick line and the edge rows of `edges` from the library's host writer -> (bytes, bytes)"""
    out, ed = folder / "want.nwk", folder / "want.csv"
    for p in (out, ed):
        if p.exists():
            p.unlink()
    pa, ch, ln = (np.ascontiguousarray(x, t) for x, t in zip(edges, (np.uint32, np.uint32, np.float64)))
    cn = (C.c_char_p * N)(*[x.encode() for x in NAMES])
    assert hiplib.tracs_tree_write(cn, N, pa.ctypes.data, ch.ctypes.data, ln.ctypes.data, len(pa), os.fsencode(str(out)), ref.encode(),
                                   os.fsencode(str(ed))) == 0
    return out.read_bytes(), ed.read_bytes()


def test_the_newick_and_the_edge_file_are_the_references(hiplib, handle, tmp_path):
    D = alignment()[1]
    got = {}
    for method, ref in (("bionj", bionj_ref.bionj), ("nj", nj_ref.nj)):
        out, ed = tmp_path / (method + ".nwk"), tmp_path / (method + ".csv")
        res = handle.tree(str(out), "x", edges_path=str(ed), method=method)
        assert (res.joins, res.rows) == (N - 3, 2 * N - 3)
        got[method] = (out.read_bytes(), ed.read_bytes())
        assert got[method] == host_files(hiplib, tmp_path, ref(D)), method
    out, ed = tmp_path / "default.nwk", tmp_path / "default.csv"
    handle.tree(str(out), "x", edges_path=str(ed))                     # (no keyword: neighbour joining, the bytes it always wrote)
    assert (out.read_bytes(), ed.read_bytes()) == got["nj"] != got["bionj"]


def test_per_site_distances_take_the_method_too(hiplib, handle, tmp_path):
    out, ed = tmp_path / "t.nwk", tmp_path / "e.csv"
    handle.tree(str(out), "x", per_site=True, edges_path=str(ed), method="bionj")      # (kind 3; no N: every pair is compared over L sites)
    assert (out.read_bytes(), ed.read_bytes()) == host_files(hiplib, tmp_path, bionj_ref.bionj(alignment()[1] / float(L)))


def test_bootstrap_replicates_are_bionj_trees(hiplib, handle, tmp_path):
    seqs, D = alignment()
    files = []
    for k in range(2):
        out, ed, reps = (tmp_path / ("%s%d" % (x, k)) for x in ("t", "e", "r"))
        handle.tree(str(out), "x", edges_path=str(ed), bootstrap=B, seed=SEED, replicate_trees=str(reps), method="bionj")
        files.append((out.read_bytes(), ed.read_bytes(), reps.read_bytes()))
    assert files[0] == files[1]                                        # reproducible for a seed
    main = bionj_ref.bionj(D)
    want = [bionj_ref.bionj(bootstrap_ref.snp_matrix(seqs, bootstrap_ref.weights(L, SEED, b)).astype(np.float64)) for b in range(B)]
    lines = files[0][2].split(b"\n")
    assert len(lines) == B + 1 and lines[-1] == b""
    for b in range(B):
        assert lines[b] + b"\n" == host_files(hiplib, tmp_path, want[b])[0], b
    support = bootstrap_ref.supports(N, main, want)
    rows = files[0][1].decode().splitlines()
    plain = host_files(hiplib, tmp_path, main)[1].decode().splitlines()
    assert len(rows) == len(plain) == 2 * N - 3
    for row, p, s in zip(rows, plain, support.tolist()):
        assert row == "%s,%s,x" % (p[:-len(",x")], "NA" if s == bootstrap_ref.NONE else str(s)), row
    assert any(0 < s < B for s in support.tolist() if s != bootstrap_ref.NONE)          # (the replicates do not all agree)


def test_tree_changes_count_on_the_bionj_edges(hiplib, handle, tmp_path):
    seqs, D = alignment()
    out, ed, si = tmp_path / "t.nwk", tmp_path / "e.csv", tmp_path / "s.csv"
    res = handle.tree(str(out), "x", edges_path=str(ed), sites_path=str(si), method="bionj")
    parent, child, length = bionj_ref.bionj(D)
    masks = bootstrap_ref.MASKS[seqs].astype(np.int64)
    want = fitch_ref.fitch(parent, child, masks)
    rows = ed.read_text().splitlines()
    assert rows[0] == "parent,child,length,changes,MSA file"
    plain = host_files(hiplib, tmp_path, (parent, child, length))[1].decode().splitlines()
    assert rows[1:] == ["%s,%d,x" % (p[:-len(",x")], c) for p, c in zip(plain, want["edge_changes"].tolist())]
    assert res.changes == want["total"] > 0


def test_the_iterated_filter_ends_on_bionj_trees(hiplib, handle, tmp_path):
    out, ed, it = tmp_path / "t.nwk", tmp_path / "e.csv", tmp_path / "i.csv"
    res = handle.tree(str(out), "x", edges_path=str(ed), tree_filter=True, iterate=3, iterations_path=str(it), method="bionj")
    assert 1 <= res.iterations <= 3 and res.joins == N - 3
    assert len(it.read_text().splitlines()) == 1 + res.iterations + 1                   # the header, a row per tree built
    nodes = nj_ref.parse_newick(out.read_text())
    assert len(nj_ref.newick_splits(nodes, NAMES)) == 2 * N - 3
    if res.masked_cells == 0:                                          # nothing was dropped: the rebuilt tree is the main BIONJ tree
        assert out.read_bytes() == host_files(hiplib, tmp_path, bionj_ref.bionj(alignment()[1]))[0]


def test_the_request_refuses_what_it_should(hiplib, handle, tmp_path):
    from tracs_amd import _lib
    o = os.fsencode(str(tmp_path / "t.nwk"))
    messages = {}
    for kind, replicates in ((1, 4), (3, 4), (4, 0), (-1, 0), (6, 0)):
        req, res = _lib.TreeRequest(kind=kind, path=o, ref=b"x", replicates=replicates, seed=1), _lib.TreeResult()
        assert hiplib.tracs_distance_tree_run(handle.h, C.byref(req), C.byref(res)) == -1
        messages[kind] = hiplib.tracs_last_error()
    assert messages[3] == messages[1] and b"SNP distance (kind 0) only" in messages[1]
    assert messages[4] == messages[-1] == messages[6] and b"kind must be" in messages[4]
    assert not os.path.exists(o)
    n_joins, rows = C.c_uint64(0), C.c_uint64(0)                       # an older entry point passes kind through
    assert hiplib.tracs_distance_tree(handle.h, _lib.TREE_BIONJ, o, b"x", None, C.byref(n_joins), C.byref(rows)) == 0
    assert open(o, "rb").read() == host_files(hiplib, tmp_path, bionj_ref.bionj(alignment()[1]))[0] and n_joins.value == N - 3
