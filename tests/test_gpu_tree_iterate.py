"""DistanceHandle.tree(iterate=K) on the GPU (tracs_distance_tree_iterate) against tests/tree_iterate_ref.py: the
iteration rows, the final tree's edges with their lengths bit for bit, its edge lists and verdicts through the change rows, and the
result.  The seeded imports' margins are checked by tests/test_tree_iterate_ref.py; the random cases' here, before anything is compared."""
import functools
import json
import os

import numpy as np
import pytest

import branch_filter_ref as bf
import hp_filter as H
import tree_iterate_ref as ti

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RANDOM = [(n, L) for n in (4, 5, 9, 33) for L in (300, 6000)]
HEADERS = {"e": "parent,child,length,changes,filtered,MSA file", "c": "parent,child,contig,position,alleleParent,alleleChild,dropped,MSA file",
           "s": "contig,position,changes,minimum,MSA file", "i": ti.ITERATIONS_HEADER}


@functools.lru_cache(maxsize=None)
def reference(kind, a, b, K, per_site=False):
    from oracle import oracle as O
    O.lib()
    masks = ti.import_case(a) if kind == "import" else ti.random_case(a, b, 100 * a + b % 7)
    return masks, ti.iterate(masks, K, O, per_site)


def run(tmp_path, masks, K, per_site=False, **kw):
    from tracs_amd.handle import DistanceHandle
    names = ["s%d" % i for i in range(masks.shape[0])]
    fa = tmp_path / "x_combined.fasta"
    ti.write_fasta(str(fa), masks, names)
    f = {k: tmp_path / (k + ".out") for k in ("o", "e", "c", "s", "f", "i")}
    with DistanceHandle([str(fa)]) as h:
        res = h.tree(str(f["o"]), "x", per_site=per_site, edges_path=str(f["e"]), changes_path=str(f["c"]), sites_path=str(f["s"]),
                     tree_filter=True, filtered_path=str(f["f"]), iterate=K, iterations_path=str(f["i"]), **kw)
    return names, f, res


def compare(names, f, res, r):
    n = len(names)
    ti.check_outputs(r, names, "x", f["o"].read_text().split("\n")[0], ti.rows_of(f["e"], "x", HEADERS["e"]), ti.rows_of(f["c"], "x", HEADERS["c"]),
                     ti.rows_of(f["s"], "x", HEADERS["s"]), f["f"].read_text().split("\n")[0], ti.rows_of(f["i"], "x", HEADERS["i"]))
    fit, _, _, kept = r["final"]
    changed = fit["site_changes"] > 0
    assert tuple(res) == (max(n - 3, 0), len(r["trees"][-1][0]), fit["total"], int(fit["site_minimum"][changed].sum()), int(kept.sum()),
                          int((kept < fit["edge_changes"]).sum()), r["iterations"], r["same_as"], r["masked_cells_last"], r["mask_work_max"])
    assert f["o"].read_text().count("\n") == 1 and f["f"].read_text().count("\n") == 1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_imports(hiplib, tmp_path, seed):
    masks, r = reference("import", seed, 0, 100)
    names, f, res = run(tmp_path, masks, 100)
    compare(names, f, res, r)
    assert res.same_as is not None and res.iterations <= 3 and res.masked_cells > 0


def test_the_limit_stops_seed_1(hiplib, tmp_path):
    masks, r = reference("import", 1, 0, 1)
    names, f, res = run(tmp_path, masks, 1)
    compare(names, f, res, r)
    assert (res.iterations, res.same_as) == (1, None)
    assert ti.rows_of(f["i"], "x", HEADERS["i"])[-1].split(",")[5:8] == ["NA", "5", "NA"]


@pytest.mark.parametrize("n,L", RANDOM, ids=["%dx%d" % s for s in RANDOM])
def test_random_alignments(hiplib, tmp_path, n, L):
    """N and partial codes present; among the cases: a repeat of T_0, cycles, and runs that reach the limit"""
    masks, r = reference("random", n, L, 4)
    assert r["margin"] > bf.MARGIN, r["margin"]
    names, f, res = run(tmp_path, masks, 4)
    compare(names, f, res, r)


def test_per_site_distances(hiplib, tmp_path):
    masks, r = reference("random", 9, 6000, 3, True)
    assert r["margin"] > bf.MARGIN and r["zero_pair"] is None
    names, f, res = run(tmp_path, masks, 3, per_site=True)
    compare(names, f, res, r)


def test_per_site_with_a_pair_left_without_sites_is_refused_by_name_and_iteration(hiplib, tmp_path):
    """samples 0 and 1 share their known sites with nobody else after the mask: s1 is N wherever s0's imported stretch is not"""
    from oracle import oracle as O
    L = 4000
    rng = np.random.default_rng(8)
    base = rng.integers(0, 4, L)
    seqs = np.tile(base, (5, 1))
    for i in range(5):
        at = rng.choice(L, 30, replace=False)
        seqs[i, at] = (base[at] + 1) % 4
    seqs[0, 1000:1060] = (base[1000:1060] + 2) % 4
    masks = (1 << seqs).astype(np.int64)
    masks[1, :1000] = 15
    masks[1, 1060:] = 15
    r = ti.iterate(masks, 3, O, True)
    assert r["zero_pair"] == 1 and r["margin"] > bf.MARGIN
    with pytest.raises(RuntimeError, match=r"iteration 1 of --tree-iterate: samples 's0' and 's1' have no site"):
        run(tmp_path, masks, 3, per_site=True)
    assert not any((tmp_path / (k + ".out")).exists() for k in "oecsfi")             # nothing was written


def test_max_entries_holds_for_every_iteration(hiplib, tmp_path):
    masks, r = reference("import", 1, 0, 100)
    assert r["rows"][0][1] < r["rows"][1][1]
    with pytest.raises(RuntimeError, match="%d changes in all, more than --max-entries %d; nothing was written" % (r["rows"][1][1], r["rows"][0][1])):
        run(tmp_path, masks, 100, max_entries=r["rows"][0][1])
    assert not any((tmp_path / (k + ".out")).exists() for k in "oecsfi")


def test_two_samples_end_on_the_pinned_filtered_count(hiplib, tmp_path):
    """[all A, one case of tests/golden/filter_hp_golden.json]: the one edge's final length is the fixture's expected count"""
    from tracs_amd.handle import DistanceHandle
    with open(os.path.join(HERE, "golden", "filter_hp_golden.json")) as fh:
        cases = [c for c in json.load(fh)["cases"] if (c["L"], c["d"]) in ((9000, 90), (9000, 600), (120000, 300))]
    assert len(cases) == 3 and any(0 < c["expected"] < c["d"] for c in cases)
    for c in cases:
        L, d = c["L"], c["d"]
        seq = np.full(L, ord("A"), np.uint8)
        seq[np.asarray(H.boundary_positions(L, d, c["row"]), np.int64)] = ord("C")
        fa = tmp_path / ("L%dd%d_combined.fasta" % (L, d))
        fa.write_bytes(b">s0\n" + b"A" * L + b"\n>s1\n" + seq.tobytes() + b"\n")
        out, ed, it = (tmp_path / ("L%dd%d.%s" % (L, d, x)) for x in ("nwk", "csv", "it"))
        with DistanceHandle([str(fa)]) as h:
            res = h.tree(str(out), "x", edges_path=str(ed), tree_filter=True, iterate=5, iterations_path=str(it))
        assert (res.iterations, res.same_as, res.changes, res.kept, res.masked_cells) == (1, 0, d, c["expected"], d - c["expected"])
        assert ed.read_text().split("\n")[1] == "s0,s1,%d,%d,%d,x" % (c["expected"], d, c["expected"])
        assert it.read_text().split("\n")[1:] == ["0,%d,%d,%d,%d,%d,NA,NA,x" % (d, c["expected"], d - c["expected"], int(c["expected"] < d), d - c["expected"]),
                                                 "1,%d,%d,%d,%d,NA,0,0,x" % (d, c["expected"], d - c["expected"], int(c["expected"] < d)), ""]


def test_without_iterate_the_entry_is_the_filter_request(hiplib, tmp_path):
    """tracs_distance_tree_iterate with it == NULL writes what tracs_distance_tree_run writes, byte for byte"""
    import ctypes as C
    from tracs_amd import _lib
    from tracs_amd.handle import DistanceHandle
    masks, _ = reference("random", 9, 300, 4)
    fa = tmp_path / "x_combined.fasta"
    ti.write_fasta(str(fa), masks)
    files = {}
    with DistanceHandle([str(fa)]) as h:
        for tag in ("run", "iterate"):
            files[tag] = [tmp_path / ("%s.%s" % (tag, k)) for k in "oecsf"]
            o, e, c, s, f = (os.fsencode(str(p)) for p in files[tag])
            req = _lib.TreeRequest(path=o, ref=b"x", edges_path=e, changes=1, changes_path=c, sites_path=s, filter=1, filtered_path=f,
                                   max_entries=10 ** 8, create=1)
            res = _lib.TreeResult()
            if tag == "run":
                _lib.check(hiplib.tracs_distance_tree_run(h.h, C.byref(req), C.byref(res)))
            else:
                _lib.check(hiplib.tracs_distance_tree_iterate(h.h, C.byref(req), None, C.byref(res), None))
            files[tag].append([getattr(res, name) for name, _ in res._fields_])
    assert files["run"][-1] == files["iterate"][-1]
    for a, b in zip(files["run"][:-1], files["iterate"][:-1]):
        assert a.read_bytes() == b.read_bytes() and a.stat().st_size > 0
