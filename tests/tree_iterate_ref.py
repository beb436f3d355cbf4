"""The branch filter iterated into the tree, restated in plain Python: the reference of tracs_alignment_mask_subtrees,
tracs_distance_tree_iterate and `tracs distance --tree nj --tree-filter --tree-iterate K`.

A: the alignment as allele masks, n x L (A = 1, C = 2, G = 4, T = 8; N = 15).  NJ(X) = nj_ref.nj of X's distances (kind 0: the sites at
which two masks are disjoint; kind 1: that over the sites at which neither is N).  V(T): fitch_ref.fitch of A on T regrouped by edge,
then branch_filter_ref.verdicts per edge.  below(T, e): the leaves in the subtree of e's child, the side away from T's top node (n = 2:
{1}).

    T_0 = NJ(A).  For k = 1 .. K:
        M_k = A with the cell (i, s) set to 15 for every dropped (e, s) of V(T_{k-1}) and every i in below(T_{k-1}, e) -- from A, never
              from M_{k-1}
        T_k = NJ(M_k)
        T_k has the non-trivial splits of some T_j, j < k: stop, same_as = the smallest such j; k = K: stop at the limit

The final tree is the last T_k; its lists and verdicts are V(T_final), from the ORIGINAL alignment.  The masked cells of tree k are the
cells that are not N in A and are N in M_{k+1}.

TEST INFRASTRUCTURE ONLY.  The seeded inputs of the GPU tests are defined here (import_case), so that the CPU test of their
conditions and the GPU tests read the same inputs.
"""
import functools

import numpy as np

import branch_filter_ref as bf
import fitch_ref
import nj_ref


def distances(masks, per_site=False):
    """-> float64 [n, n], or None when per_site and some pair is compared over 0 sites"""
    m = np.asarray(masks, np.int64)
    n = m.shape[0]
    D = np.zeros((n, n), np.float64)
    known = m != 15
    for i in range(n):
        d = ((m[i][None, :] & m) == 0).sum(axis=1).astype(np.float64)
        if per_site:
            nn = (known[i][None, :] & known).sum(axis=1).astype(np.float64)
            if (np.delete(nn, i) == 0).any():
                return None
            nn[i] = 1.0
            d = d / nn
        D[i] = d
    np.fill_diagonal(D, 0.0)
    return D


def below(n, parent, child):
    """-> [sorted leaves below the child of edge e] for every edge"""
    parent, child = [int(x) for x in parent], [int(x) for x in child]
    if n == 2:
        return [[1]]
    under = {i: [i] for i in range(n)}
    for p, c in zip(parent, child):                                # creation order: a child is complete before its parent's rows
        under.setdefault(p, [])
        under[p] = under[p] + under[c]
    return [sorted(under[c]) for c in child]


def splits(n, parent, child):
    """the set of non-trivial splits of a tree in creation order (empty for n < 4)"""
    if n < 4:
        return frozenset()
    s = nj_ref.splits_of(n, np.asarray(parent), np.asarray(child), np.zeros(len(parent)))
    full = (1 << n) - 1
    return frozenset(m for m in s if bin(m).count("1") >= 2 and bin(full & ~m).count("1") >= 2)


def filtered(parent, child, masks, oracle):
    """V(T): -> (fitch dict, lists, [bool array kept? per entry of edge e], kept per edge)"""
    L = np.asarray(masks).shape[1]
    r, lists = bf.edge_lists(parent, child, masks)
    keep = [bf.verdicts(x, L, oracle) for x in lists]
    return r, lists, keep, np.array([int(k.sum()) for k in keep], np.int64)


def mask(masks, parent, child, lists, keep):
    """M: `masks` with 15 at (i, s) for every dropped (e, s) and every i below e -> (M, the cells newly 15, the work W)"""
    masks = np.asarray(masks, np.int64)
    M = masks.copy()
    work = 0
    for leaves, sites, kept in zip(below(masks.shape[0], parent, child), lists, keep):
        drop = np.asarray(sites, np.int64)[~np.asarray(kept, bool)]
        work += len(drop) * len(leaves)
        if len(drop):
            M[np.ix_(leaves, drop)] = 15
    return M, int(((masks != 15) & (M == 15)).sum()), work


def iterate(masks, K, oracle, per_site=False):
    """-> dict: rows [(k, changes, kept, dropped, branches with a drop, masked cells or None, shared splits or None, same as or None)],
    trees [(parent, child, length)] for k = 0 .. final, M [None, M_1, ..], final (fitch dict, lists, keep, kept per edge), iterations,
    same_as (None: stopped at the limit), masked_cells_last, mask_work_max, margin (the smallest over every iteration's lists);
    zero_pair: the iteration whose kind-1 matrix has a pair compared over 0 sites (the run is refused there), else None"""
    masks = np.asarray(masks, np.int64)
    n, L = masks.shape
    out = {"rows": [], "trees": [nj_ref.nj(distances(masks, per_site))], "M": [None], "zero_pair": None, "margin": 1.0,
           "masked_cells_last": 0, "mask_work_max": 0}
    k, stop, same, shared = 0, False, None, None
    while True:
        parent, child, _ = out["trees"][k]
        r, lists, keep, kept = filtered(parent, child, masks, oracle)
        out["margin"] = min([out["margin"]] + [bf.margin(x, L, oracle) for x in lists])
        row = [k, r["total"], int(kept.sum()), r["total"] - int(kept.sum()), int((kept < r["edge_changes"]).sum()), None, shared, None]
        if stop:
            row[7] = same
            out["rows"].append(tuple(row))
            out["final"] = (r, lists, keep, kept)
            break
        M, cells, work = mask(masks, parent, child, lists, keep)
        row[5] = cells
        out["rows"].append(tuple(row))
        out["masked_cells_last"], out["mask_work_max"] = cells, max(out["mask_work_max"], work)
        k += 1
        D = distances(M, per_site)
        if D is None:
            out["zero_pair"] = k
            break
        out["M"].append(M)
        out["trees"].append(nj_ref.nj(D))
        mine = splits(n, *out["trees"][k][:2])
        earlier = [splits(n, *t[:2]) for t in out["trees"][:k]]
        same = next((j for j, s in enumerate(earlier) if s == mine), None)
        shared = len(mine & earlier[-1])
        stop = same is not None or k == K
    out["iterations"], out["same_as"] = k, same
    return out


def row_text(row, ref):
    """one row of --tree-iterate-out"""
    return ",".join("NA" if v is None else str(v) for v in row) + "," + ref


# ---- the seeded inputs of tests/test_gpu_tree_iterate*.py ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def import_case(seed):
    """-> masks (int64 [10, 20000], read-only): two clades {0..4} and {5..9} separated by 60 sites, 25 of them inside the window
    [7000, 7200) and 35 outside [6900, 7300); shared sites outside the window: 6 each for {0, 1}, {2, 3}, {5, 6}, {7, 8} and 5 for
    {7, 8, 9}; 10 private sites per sample outside the window; then sample 2 takes sample 7's bases over [7000, 7200).  A mutation is
    base + 1 mod 4; every mutated site is distinct."""
    rng = np.random.default_rng(seed)
    n, L = 10, 20000
    base = rng.integers(0, 4, L)
    seqs = np.tile(base, (n, 1))
    inside = np.arange(7000, 7200)
    outside = np.concatenate([np.arange(0, 6900), np.arange(7300, L)])
    groups = [(list(range(5, 10)), 25, inside), (list(range(5, 10)), 35, outside)]
    groups += [(g, 6, outside) for g in ([0, 1], [2, 3], [5, 6], [7, 8])] + [([7, 8, 9], 5, outside)]
    groups += [([i], 10, outside) for i in range(n)]
    used = np.zeros(L, bool)
    for samples, count, where in groups:
        free = where[~used[where]]
        sites = rng.choice(free, count, replace=False)
        used[sites] = True
        seqs[np.ix_(samples, sites)] = (base[sites] + 1) % 4
    seqs[2, 7000:7200] = seqs[7, 7000:7200]
    masks = (1 << seqs).astype(np.int64)
    masks.setflags(write=False)
    return masks


def random_case(n, L, seed):
    """a few lineages, private mutations, N, partial codes, and an imported stretch on one sample"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, L)
    lineage = np.where(rng.random((3, L)) < 0.03, rng.integers(0, 4, (3, L)), base)
    pick = rng.integers(0, 3, n)
    seqs = np.where(rng.random((n, L)) < 0.01, rng.integers(0, 4, (n, L)), lineage[pick])
    a, w = L // 3, min(60, L // 5)
    seqs[n - 1, a:a + w] = (lineage[(pick[n - 1] + 1) % 3, a:a + w] + 1 + np.arange(w) % 2) % 4
    masks = (1 << seqs).astype(np.int64)
    masks = np.where(rng.random((n, L)) < 0.02, 15, masks)
    masks = np.where(rng.random((n, L)) < 0.005, rng.integers(1, 16, (n, L)), masks)
    return masks.astype(np.int64)


def text(masks):
    """the canonical letters of the masks, uint8 [n, L]"""
    return np.ascontiguousarray(np.frombuffer(fitch_ref.LETTERS.encode(), np.uint8)[np.asarray(masks)])


def write_fasta(path, masks, names=None):
    t = text(masks)
    with open(path, "wb") as fh:
        for i, row in enumerate(t):
            fh.write(b">" + (names[i] if names else "s%d" % i).encode() + b"\n" + row.tobytes() + b"\n")


# ---- the files of a run against the reference ------------------------------------------------------------------------------------------
ITERATIONS_HEADER = "iteration,changes,kept,dropped,branches with a drop,masked cells,shared splits,same as,MSA file"


def rows_of(path, ref, header):
    """the rows of one --msa file in a file that several runs appended to: header checked, rows ending in `ref`"""
    lines = open(path).read().split("\n")
    assert lines[0] == header and lines[-1] == "" and lines.count(header) == 1, path
    return [ln for ln in lines[1:-1] if ln.endswith("," + ref)]


def check_outputs(r, names, ref, newick, edge_rows, change_rows, site_rows, filtered, iter_rows):
    """every file of a run (each None, or its lines for this --msa file) against iterate()'s result: exact, the lengths bit for bit"""
    n = len(names)
    parent, child, length = r["trees"][-1]
    fit, lists, keep, kept = r["final"]
    name = lambda v: names[v] if v < n else "#%d" % (v - n + 1)                         # noqa: E731
    if iter_rows is not None:
        assert iter_rows == [row_text(row, ref) for row in r["rows"]]
    if edge_rows is not None:
        rows = [x.split(",") for x in edge_rows]
        assert [x[:2] + x[3:] for x in rows] == [[name(int(p)), name(int(c)), str(int(ch)), str(int(k)), ref]
                                                  for p, c, ch, k in zip(parent, child, fit["edge_changes"], kept)]
        got = np.array([float(x[2]) for x in rows], np.float64)
        assert np.array_equal(got.view(np.uint64), np.asarray(length, np.float64).view(np.uint64)), (got, length)
    for line, lengths in ((newick, length), (filtered, kept.astype(np.float64))):
        if line is not None and n >= 3:
            got = nj_ref.newick_splits(nj_ref.parse_newick(line), names)
            want = nj_ref.splits_of(n, parent, child, np.asarray(lengths, np.float64))
            assert got == want
    if change_rows is not None:
        letter = {1: "A", 2: "C", 4: "G", 8: "T"}
        dropped = {(int(s), e): not bool(k) for e, (sites, ks) in enumerate(zip(lists, keep)) for s, k in zip(sites, ks)}
        assert change_rows == ["%s,%s,alignment,%d,%s,%s,%d,%s" % (name(int(parent[e])), name(int(child[e])), s, letter[info & 15], letter[info >> 4],
                                                                 int(dropped[(s, e)]), ref) for s, e, info in fit["entries"]]
    if site_rows is not None:
        assert site_rows == ["alignment,%d,%d,%d,%s" % (s, int(fit["site_changes"][s]), int(fit["site_minimum"][s]), ref)
                             for s in np.flatnonzero(fit["site_changes"])]
