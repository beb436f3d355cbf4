"""The float64 panel stage of `tracs cluster -D direct|expectedK -c T` against numpy: tracs_edges_count_f64 / _fill_f64
(device.edges_from_dense_f64), tracs_coo_fill_f64, the panel form of device.trans_dist_dense (absolute row numbers through
base_row), and multigpu.edges_of_rank / cluster_edges with the ranks played one after the other in this process.

The kept cells are  (j > i) & (j >= col_begin) & (row_begin <= i < row_end) & (dist as uint32 <= dist_threshold) & (val <= threshold),
row-major: the reference's `float(line[col]) <= args.threshold` on the emitted pairs (tracs/cluster.py:110-112)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_keysplit import _matrix  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = 2147483647
INF = float("inf")


def _kept(val, dist, n, threshold, dist_threshold=BIG, row_begin=0, row_end=None, col_begin=0):
    """numpy: rows, cols (int32, row-major) and values of the kept cells; val / dist: [n, n] float64 / uint32"""
    row_end = n if row_end is None else row_end
    i, j = np.mgrid[0:n, 0:n]
    with np.errstate(invalid="ignore"):
        keep = (j > i) & (j >= col_begin) & (i >= row_begin) & (i < row_end) & (dist.astype(np.int64) <= dist_threshold) & (val <= threshold)
    r, c = np.nonzero(keep)
    return r.astype(np.int32), c.astype(np.int32), val[r, c]


def _inputs(n, seed):
    """values of both signs (a few NaN, +-inf, +-0 among them) and distances 0..40 with cells of 0xFFFFFFFF (what
    tracs_pairsnp_dense_thr leaves beyond its threshold)"""
    rng = np.random.default_rng(seed)
    val = rng.normal(size=(n, n))
    special = rng.random((n, n))
    for lo, v in ((0.00, np.nan), (0.02, np.inf), (0.04, -np.inf), (0.06, 0.0), (0.08, -0.0), (0.10, 0.25)):
        val[(special >= lo) & (special < lo + 0.02)] = v
    dist = rng.integers(0, 41, size=(n, n)).astype(np.uint32)
    dist[rng.random((n, n)) < 0.1] = 0xFFFFFFFF
    return val, dist


def _device(val, dist, ld, rows=None):
    """[rows, ld] device buffers holding the rows `rows` (default: all) of val / dist in their first n columns; the padding columns
    and nothing else look like kept cells (value -1, distance 0) -> (val view [rows, n], dist view as int32)"""
    import torch
    n = val.shape[1]
    r0, r1 = rows if rows is not None else (0, val.shape[0])
    vb = torch.full((r1 - r0, ld), -1.0, dtype=torch.float64, device="cuda")
    db = torch.zeros((r1 - r0, ld), dtype=torch.int32, device="cuda")
    vb[:, :n] = torch.from_numpy(val[r0:r1]).cuda()
    db[:, :n] = torch.from_numpy(dist[r0:r1].view(np.int32)).cuda()
    return vb[:, :n], db[:, :n]


def _run(dev, vd, dd, n, threshold, want, with_values, **kw):
    """edges_from_dense_f64 against the expected (rows, cols, values): the count, and every element, exactly"""
    got = dev.edges_from_dense_f64(vd, dd, n, threshold, with_values=with_values, **kw)
    assert len(got) == (3 if with_values else 2)
    assert got[0].numel() == got[1].numel() == len(want[0]), (got[0].numel(), len(want[0]), kw)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]), kw
    if with_values:
        assert np.array_equal(got[2].cpu().numpy().view(np.uint64), want[2].view(np.uint64)), kw


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 66, 129, 200])
def test_edges_match_numpy(n, pad):
    """Sizes around the 64 columns a wave takes per step, ld = n and n + 5, every column bound, with and without values, the
    whole matrix and a row range inside it, finite and infinite thresholds, a distance threshold among the distances."""
    from tracs_amd import device as dev
    val, dist = _inputs(n, 100 + n)
    vd, dd = _device(val, dist, n + pad)
    kept_some = False
    for cb in sorted({0, 1, 64, 70, max(0, n - 1), n}):
        for rows in ((0, n), (n // 3, max(n // 3, n - 1))):
            for threshold, dthr in ((0.25, BIG), (INF, 20), (-0.5, 20)):
                want = _kept(val, dist, n, threshold, dthr, rows[0], rows[1], cb)
                kept_some |= 0 < len(want[0])
                for wv in (False, True):
                    _run(dev, vd, dd, n, threshold, want, wv, dist_threshold=dthr, row_begin=rows[0], row_end=rows[1], col_begin=cb)
    assert kept_some or n <= 2


@pytest.mark.parametrize("rows", [(1, 1024), (0, 1024), (1, 1026), (0, 1026)])
def test_offsets_cross_the_scan_tile(rows):
    """n = 1026: the n + 1 offsets of 1023, 1024, 1025 and 1026 rows around the 1024 entries scan_i64_inplace_kernel takes per step."""
    from tracs_amd import device as dev
    n = 1026
    val, dist = _inputs(n, 7)
    vd, dd = _device(val, dist, n)
    want = _kept(val, dist, n, 0.25, 30, rows[0], rows[1], 0)
    assert 0 < len(want[0])
    _run(dev, vd, dd, n, 0.25, want, True, dist_threshold=30, row_begin=rows[0], row_end=rows[1])


def test_panel_tensor_with_base_row():
    """A tensor that holds only the rows 70..150 of 200 samples, indexed by absolute row numbers (base_row = 70)."""
    from tracs_amd import device as dev
    n = 200
    val, dist = _inputs(n, 11)
    for pad in (0, 5):
        vd, dd = _device(val, dist, n + pad, rows=(70, 150))
        for rows in ((70, 150), (71, 149), (100, 100)):
            for cb in (0, 64, 120):
                want = _kept(val, dist, n, 0.25, 30, rows[0], rows[1], cb)
                assert (len(want[0]) > 0) == (rows[0] < rows[1])
                for wv in (False, True):
                    _run(dev, vd, dd, n, 0.25, want, wv, dist_threshold=30, row_begin=rows[0], row_end=rows[1], col_begin=cb, base_row=70)


def test_empty_results():
    import torch
    from tracs_amd import device as dev
    n = 66
    val = np.full((n, n), 1.0)
    dist = np.zeros((n, n), np.uint32)
    vd, dd = _device(val, dist, n)
    for kw in (dict(threshold=0.5), dict(threshold=1.0, row_begin=20, row_end=20), dict(threshold=1.0, col_begin=n),
               dict(threshold=1.0, dist_threshold=-1), dict(threshold=-INF)):
        threshold = kw.pop("threshold")
        for wv in (False, True):
            got = dev.edges_from_dense_f64(vd, dd, n, threshold, with_values=wv, **kw)
            assert [g.numel() for g in got] == [0] * len(got) and got[0].dtype == torch.int32 and got[1].dtype == torch.int32
    # ... and the same matrix at its own value: every cell of the upper triangle
    assert dev.edges_from_dense_f64(vd, dd, n, 1.0)[0].numel() == n * (n - 1) // 2


def test_values_at_the_threshold():
    """Planted at known cells: exactly the threshold (kept), the next double above it (dropped), NaN (dropped), -inf (kept), +inf
    against a finite threshold (dropped); -0.0 against a threshold of 0.0 (kept); threshold = +inf keeps every finite value and +inf,
    never NaN."""
    from tracs_amd import device as dev
    n, t = 129, 0.3125
    rng = np.random.default_rng(3)
    val = t + 1.0 + rng.random((n, n))                               # everything else: above the threshold
    dist = np.zeros((n, n), np.uint32)
    cells = {(0, 1): t, (0, 64): np.nextafter(t, INF), (0, 65): np.nan, (5, 128): -INF, (63, 64): INF, (64, 65): np.nextafter(t, -INF),
             (64, 128): -0.0, (127, 128): 0.0, (70, 71): 5e-324, (70, 72): -5e-324}
    for (i, j), v in cells.items():
        val[i, j] = v
        val[j, i] = t                                                  # (below the diagonal: never an edge)
    vd, dd = _device(val, dist, n)

    def kept(threshold):
        r, c, v = dev.edges_from_dense_f64(vd, dd, n, threshold, with_values=True)
        r, c, v = r.cpu().numpy(), c.cpu().numpy(), v.cpu().numpy()
        want = _kept(val, dist, n, threshold)
        assert np.array_equal(r, want[0]) and np.array_equal(c, want[1]) and np.array_equal(v.view(np.uint64), want[2].view(np.uint64))
        return set(zip(r.tolist(), c.tolist()))

    assert kept(t) == {(0, 1), (5, 128), (64, 65), (64, 128), (127, 128), (70, 71), (70, 72)}
    assert kept(0.0) == {(5, 128), (64, 128), (127, 128), (70, 72)}
    assert kept(-0.0) == {(5, 128), (64, 128), (127, 128), (70, 72)}
    assert kept(-INF) == {(5, 128)}
    everything = {(i, j) for i in range(n) for j in range(i + 1, n)}
    assert kept(INF) == everything - {(0, 65)}
    assert kept(float("nan")) == set()


def test_distance_threshold():
    """0xFFFFFFFF (a pair beyond tracs_pairsnp_dense_thr's threshold) is dropped at 2147483647; a distance equal to the threshold is
    kept, one above it dropped; 0 keeps the zero-distance cells; -1 keeps nothing."""
    from tracs_amd import device as dev
    n = 66
    val = np.zeros((n, n))
    dist = np.full((n, n), 9, np.uint32)
    dist[0, 1], dist[0, 65], dist[1, 2], dist[3, 64], dist[64, 65], dist[2, 3] = 0xFFFFFFFF, 7, 8, 0, 0x80000000, 2147483647
    vd, dd = _device(val, dist, n)

    def kept(dthr):
        r, c = dev.edges_from_dense_f64(vd, dd, n, 0.0, dist_threshold=dthr)
        want = _kept(val, dist, n, 0.0, dthr)
        assert np.array_equal(r.cpu().numpy(), want[0]) and np.array_equal(c.cpu().numpy(), want[1])
        return set(zip(r.cpu().numpy().tolist(), c.cpu().numpy().tolist()))

    everything = {(i, j) for i in range(n) for j in range(i + 1, n)}
    assert kept(BIG) == everything - {(0, 1), (64, 65)}
    assert kept(7) == {(0, 65), (3, 64)}
    assert kept(8) == {(0, 65), (1, 2), (3, 64)}
    assert kept(0) == {(3, 64)}
    assert kept(-1) == set()


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 66, 129, 200])
def test_coo_fill_f64_matches_numpy(n, pad):
    """tracs_coo_fill_f64 with tracs_coo_count's offsets: out_a[k], out_b[k] = a, b at the k-th cell within the distance threshold,
    bit for bit (any bit pattern), and the element behind the last one is left alone."""
    import torch
    from tracs_amd import _lib
    from tracs_amd import device as dev
    L = _lib.load()
    rng = np.random.default_rng(200 + n)
    _, dist = _inputs(n, 300 + n)
    a = rng.integers(0, 1 << 63, size=(n, n), dtype=np.int64).view(np.float64)      # every bit pattern: NaN payloads, denormals
    b = rng.integers(0, 1 << 63, size=(n, n), dtype=np.int64).view(np.float64)
    everything = np.full((n, n), -1.0)
    ld = n + pad
    sentinel = -12345.0
    for base_row, rows_held in ((0, (0, n)), (n // 3, (n // 3, n))):
        ad, dd = _device(a, dist, ld, rows=rows_held)
        bd, _ = _device(b, dist, ld, rows=rows_held)
        for cb in sorted({0, 1, 64, 70, max(0, n - 1), n}):
            for rows in ((rows_held[0], n), (rows_held[0], rows_held[0]), (min(n, rows_held[0] + 1), max(min(n, rows_held[0] + 1), n - 1))):
                for dthr in (BIG, 20, -1):
                    r, c, _ = _kept(everything, dist, n, 0.0, dthr, rows[0], rows[1], cb)
                    got = dev.coo_from_dense(dd, None, n, dthr, row_begin=rows[0], row_end=rows[1], col_begin=cb, base_row=base_row)
                    assert np.array_equal(got[0].cpu().numpy(), r) and np.array_equal(got[1].cpu().numpy(), c)
                    nrows = max(0, rows[1] - rows[0])
                    off = torch.zeros(nrows + 1, dtype=torch.int64, device="cuda")
                    _lib.check(L.tracs_coo_count(dev._panel_ptr(dd, base_row), ld, n, rows[0], rows[1], cb, dthr, dev._ptr(off), dev._stream()))
                    assert int(off[nrows].item()) == len(r)
                    oa = torch.full((len(r) + 1,), sentinel, dtype=torch.float64, device="cuda")
                    ob = torch.full((len(r) + 1,), sentinel, dtype=torch.float64, device="cuda")
                    _lib.check(L.tracs_coo_fill_f64(dev._panel_ptr(dd, base_row), ld, n, rows[0], rows[1], cb, dthr, dev._ptr(off),
                                                    dev._panel_ptr(ad, base_row), dev._panel_ptr(bd, base_row), dev._ptr(oa), dev._ptr(ob),
                                                    dev._stream()))
                    oa, ob = oa.cpu().numpy(), ob.cpu().numpy()
                    assert oa[-1] == sentinel and ob[-1] == sentinel
                    assert np.array_equal(oa[:-1].view(np.uint64), a[r, c].view(np.uint64))
                    assert np.array_equal(ob[:-1].view(np.uint64), b[r, c].view(np.uint64))


# ---- the panel form of trans_dist_dense ------------------------------------------------------------------------------------------
LAMB, BETA, PREC = 5.3, 6.0, 0.01


def test_trans_dist_dense_panels_equal_the_whole_matrix():
    """333 samples in panels of 64 rows, each handed over as its own [64, n] tensors with base_row = its first row: stitched
    together they equal the one call over the whole matrix bit for bit, and the rows of the last panel's tensors beyond the matrix
    keep their fill.  Within dist_threshold = 60 the distances are 12..36, far below the 128 from which a key's series is summed
    from the prefix tables: a key's value must not depend on the other keys of its call.  The whole matrix and the first panels
    have enough keys (2 048) for those tables, the last panels do not -- both kinds of call are asserted to occur."""
    import torch
    from tracs_amd import device as dev
    n, R, thr = 333, 64, 60
    d, days = _matrix(n, 21)
    dm, dy = torch.from_numpy(d).cuda(), torch.from_numpy(days).cuda()
    nan = float("nan")
    p = torch.full((n, n), nan, dtype=torch.float64, device="cuda")
    e = torch.full((n, n), nan, dtype=torch.float64, device="cuda")
    dev.trans_dist_dense(dm, n, dy, LAMB, BETA, PREC, p, e, exp_p0=True, dist_threshold=thr)
    assert dev.trans_routes()["tables"]
    tabled = set()
    i, j = np.mgrid[0:n, 0:n]
    valid = (j > i) & (d <= thr)
    assert valid.any() and (~valid & (j > i)).any()
    assert np.array_equal(~np.isnan(p.cpu().numpy()), valid) and np.array_equal(~np.isnan(e.cpu().numpy()), valid)
    for r0 in range(0, n, R):
        r1 = min(n, r0 + R)
        dpan = torch.full((R, n), 20, dtype=torch.int32, device="cuda")          # (rows beyond the panel look like valid cells)
        dpan[:r1 - r0] = dm[r0:r1]
        ppan = torch.full((R, n), nan, dtype=torch.float64, device="cuda")
        epan = torch.full((R, n), nan, dtype=torch.float64, device="cuda")
        dev.trans_dist_dense(dpan, n, dy, LAMB, BETA, PREC, ppan, epan, exp_p0=True, dist_threshold=thr, row_begin=r0, row_end=r1,
                             base_row=r0)
        tabled.add(dev.trans_routes()["tables"])
        for whole, pan in ((p, ppan), (e, epan)):
            assert np.array_equal(pan[:r1 - r0].cpu().numpy().view(np.uint64), whole[r0:r1].cpu().numpy().view(np.uint64)), (r0, r1)
            assert bool(torch.isnan(pan[r1 - r0:]).all())
    assert tabled == {True, False}, tabled


# ---- edges_of_rank / cluster_edges -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cluster_case():
    """300 samples in three tight groups, a SNP threshold of 100 that drops some of the pairs between groups: P and E(K) of the
    whole matrix in one call, once for every test below."""
    import torch
    from tracs_amd import device as dev
    n, dthr = 300, 100
    d, days = _matrix(n, 31)
    dm, dy = torch.from_numpy(d).cuda(), torch.from_numpy(days).cuda()
    p = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
    e = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
    dev.trans_dist_dense_ranges(dm, n, dy, LAMB, BETA, PREC, p, e, [(0, n)], exp_p0=True, dist_threshold=dthr)
    return dict(n=n, dthr=dthr, d=d, dm=dm, dy=dy, direct=p.cpu().numpy(), expectedK=e.cpu().numpy())


@pytest.mark.parametrize("column", ["expectedK", "direct"])
def test_edges_of_rank_and_components(cluster_case, column, monkeypatch):
    """Worlds of 1 and 3 ranks, every rank in turn in this process (no torch.distributed), with the default panel size (a chunk is one
    panel) and with multigpu.panel_rows giving 64 (a chunk of world 1 spans several panels, base_row != 0): the chunks' edges in
    chunk order equal the numpy rule on the whole-matrix values, and the components equal SciPy's labels (tracs/cluster.py:126-129).
    The value threshold lies halfway between two neighbouring values of the matrix, three tenths of the way up.
    cluster_edges itself runs for world = 1 (partition.gather_coo needs no process group there); for world = 3 the component
    kernel runs on the concatenated chunks, which is what rank 0 holds after the gather."""
    import torch
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    from tracs_amd import device as dev
    from tracs_amd import multigpu
    from tracs_amd import partition
    c = cluster_case
    n, dthr, val, du = c["n"], c["dthr"], c[column], c["d"].view(np.uint32)
    iu = np.triu_indices(n, 1)
    emitted = c["d"][iu] <= dthr
    assert emitted.any() and (~emitted).any()                          # the SNP threshold keeps some pairs and drops some
    vs = np.unique(val[iu][emitted])
    assert not np.isnan(vs).any() and len(vs) > 10
    k = int(0.3 * len(vs))
    threshold = 0.5 * (float(vs[k]) + float(vs[k + 1]))
    rows, cols, _ = _kept(val, du, n, threshold, dthr)
    assert 0 < len(rows) < int(emitted.sum())                          # ... and so does the value threshold
    want_nc, want_lab = connected_components(csgraph=csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)), directed=False)
    assert want_nc < n
    print("%s: threshold %.6g keeps %d of %d emitted pairs, %d components" % (column, threshold, len(rows), int(emitted.sum()), want_nc))

    def dist_fn(dpan, npan, r0, r1):
        dpan[:r1 - r0].copy_(c["dm"][r0:r1])

    for patched in (False, True):
        if patched:
            monkeypatch.setattr(multigpu, "panel_rows", lambda n, budget_bytes=0: 64)
        for world in (1, 3):
            chunks = {}
            for rank in range(world):
                parts = multigpu.edges_of_rank(dist_fn, n, c["dy"], LAMB, BETA, PREC, column, threshold, rank, world, dist_threshold=dthr)
                assert sorted(parts) == sorted(set(partition.rank_chunks(rank, world)))
                for ch, (r, cc) in parts.items():
                    assert ch not in chunks and r.dtype == torch.int32 and cc.dtype == torch.int32
                    rn, cn = r.cpu().numpy().astype(np.int64), cc.cpu().numpy().astype(np.int64)
                    assert (np.diff(rn * n + cn) > 0).all()            # row-major within the chunk
                    chunks[ch] = (r, cc)
                if world == 1:
                    nc, lab = multigpu.cluster_edges(parts, n, 0, 1, None)
                    assert nc == want_nc and np.array_equal(lab.cpu().numpy(), want_lab)
            I = torch.cat([chunks[ch][0] for ch in sorted(chunks)])
            J = torch.cat([chunks[ch][1] for ch in sorted(chunks)])
            assert np.array_equal(I.cpu().numpy(), rows) and np.array_equal(J.cpu().numpy(), cols), (world, patched)
            nc, lab = dev.connected_components_device(I, J, n)
            assert nc == want_nc and np.array_equal(lab.cpu().numpy(), want_lab), (world, patched)
