"""Every GPU route of the pair loop and of the recombination filter against what the reference's own src/pairsnp.hpp returned
(tests/golden/pairsnp_ref_golden.npz; generator: tests/golden/make_golden.py pairsnp-ref; layout: tests/pairsnp_ref_cases.py).
Only the stored fixture is read: neither the reference nor oracle/_ref, and the oracle decides nothing here.  All comparisons
are exact: rows, cols, d, compared sites and filtered d are integers, and the generator found no window of any filter case within
1e-9 (relative) of its threshold.

Pair loop: api.pairsnp_arrays from the FASTA files (pack, thresholds, two files, wrapped / CRLF / gzip); dev.pairsnp_dense under the
kernel switches of tests/test_gpu_kernel_variants.py, each in a child process that reports the kernel it ran
(tests/pairsnp_ref_gpu_child.py).  Filter: dev.filter_recomb_pairs on the routes of tests/test_gpu_filter_hp.py,
dev.filter_recomb_device, dev.filter_recomb_lists on the position lists, and api.pairsnp_arrays(filter=True)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

import pairsnp_ref_cases as PC  # noqa: E402
from test_gpu_filter_hp import ALL_ROUTES  # noqa: E402

META, ARRAYS = PC.load()
PAIR_CASES = {c["name"]: c for c in META["cases"]}
FILTER_CASES = {c["name"]: c for c in META["filter_cases"]}


def _api_case(case, tmp_path):
    from tracs_amd import api
    seqs = ARRAYS["aln/" + case["aln"]]
    fastas = PC.write_fastas(case, seqs, str(tmp_path))
    r, c, d, names, filt, nn = api.pairsnp_arrays(fastas, 1, case["dist"], case["filter"])
    want = PC.expected(ARRAYS, case)
    assert list(names) == PC.names_of(seqs.shape[0])
    for what, g, w in zip(PC.COLUMNS, (r, c, d, nn, filt), want):
        g = np.asarray(g).astype(np.int64)
        assert g.shape == w.shape and np.array_equal(g, w), (case["name"], what, g.shape, w.shape)
    return want


@pytest.mark.parametrize("name", sorted(PAIR_CASES))
def test_pairsnp_from_fasta_equals_the_reference(hiplib, tmp_path, name):
    """rows, cols, d, nn in the reference's order, and a zero per pair in the filtered column (filter = False)"""
    want = _api_case(PAIR_CASES[name], tmp_path)
    assert not want[4].any()


# the routes of tests/test_gpu_kernel_variants.py the pair loop can take: (switches, the kernel of a consensus / of a general
# alignment, site classes: True forced on, False off, None the library's choice)
DENSE_ROUTES = {
    "default": ({}, "mfma", "mfma-general", None),
    "classes_off": ({"TRACS_SITE_CLASSES": "0"}, "mfma", "mfma-general", False),
    "classes_on": ({"TRACS_SITE_CLASSES": "1"}, "mfma", "mfma-general", True),
    "classes_on_ksplit3": ({"TRACS_SITE_CLASSES": "1", "TRACS_KSPLIT": "3"}, "mfma", "mfma-general", True),
    "valu_tile": ({"TRACS_MFMA": "0"}, "valu", "valu", False),
    "valu_tile3_ksplit3": ({"TRACS_TILE_VARIANT": "3", "TRACS_KSPLIT": "3"}, "valu", "valu", False),
    "ksplit4_supertile": ({"TRACS_KSPLIT": "4", "TRACS_SUPERTILE": "2x2"}, "mfma", "mfma-general", None),
    "count_in_place": ({"TRACS_COUNT_IN_PLACE": "1"}, "mfma", "mfma-general", None),
    "count_in_place_ksplit3": ({"TRACS_COUNT_IN_PLACE": "1", "TRACS_KSPLIT": "3"}, "mfma", "mfma-general", None),
}
# the alignments whose encoding their content decides: N only -> consensus; a few partial codes -> general on the matrix cores (the
# small ones dense in partial codes -- iupac_small, len_*, and tail_129 without site classes -- have sparse lists too dense for the
# correction and take the VALU tile whatever the switches say: the library's documented choice, not a fall-back)
CONSENSUS, GENERAL = ("consensus_300",), ("n70", "n130")


@pytest.mark.parametrize("route", sorted(DENSE_ROUTES))
def test_pairsnp_dense_equals_the_reference_on_every_kernel_route(hiplib, route):
    env, k_consensus, k_general, classes = DENSE_ROUTES[route]
    out = subprocess.run([sys.executable, os.path.join(HERE, "pairsnp_ref_gpu_child.py")], capture_output=True, text=True,
                         env=dict(os.environ, **env), timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
    used = {}
    for ln in out.stdout.splitlines():
        if ln.startswith("USED "):
            _, aln, enc, kern, cls = ln.split()
            used.setdefault(aln, set()).add((enc, kern, cls == "1"))
    assert set(used) == {c["aln"] for c in META["cases"]}
    # no route falls back silently: the kernel and the encoding of the alignments whose encoding their content decides
    for aln in CONSENSUS:
        assert {(e, k) for e, k, _ in used[aln]} == {("consensus", k_consensus)}, (route, aln, used[aln])
    for aln in GENERAL:
        assert {(e, k) for e, k, _ in used[aln]} == {("general", k_general)}, (route, aln, used[aln])
    if classes is not None:
        for aln in CONSENSUS + GENERAL:
            assert {c for _, _, c in used[aln]} == {classes}, (route, aln, used[aln])
    else:
        assert any(c for v in used.values() for _, _, c in v), (route, used)


def _packed(name):
    from tracs_amd import device as dev
    seqs = ARRAYS["aln/" + name]
    aln = dev.Alignment(*seqs.shape)
    aln.pack(seqs)
    return aln


def _dev(*cols):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda() for x in cols]


@pytest.mark.parametrize("route", sorted(ALL_ROUTES))
def test_filter_recomb_pairs_equals_the_reference_on_every_route(hiplib, monkeypatch, route):
    """filtered d of every emitted pair of the planted-import alignments: all pairs, then a subset, then all in reverse"""
    from tracs_amd import device as dev
    for k, v in ALL_ROUTES[route].items():
        monkeypatch.setenv(k, v)
    for name, case in sorted(FILTER_CASES.items()):
        r, c, d, _, filt = PC.expected(ARRAYS, case)
        assert (filt < d).any() and (filt <= d).all()
        aln = _packed(case["aln"])
        for o in (np.arange(len(r)), np.arange(len(r))[1::3], np.arange(len(r))[::-1]):
            got = dev.filter_recomb_pairs(aln, *_dev(r[o], c[o], d[o])).cpu().numpy()
            assert np.array_equal(got, filt[o]), (route, name, np.nonzero(got != filt[o])[0][:8])
        info = dev.filter_index_info(aln)
        assert info is not None and info["lists"] == (not route.startswith("scan")), (route, name, info)
        aln.close()


@pytest.mark.parametrize("lanes_min", ["0", "1000000000000"], ids=["pair_per_lane", "wave_per_pair"])
def test_filter_recomb_device_equals_the_reference(hiplib, monkeypatch, lanes_min):
    """the plane scan with its positions: filtered d, and as many SNP sites found per pair as the reference's d"""
    from tracs_amd import device as dev
    monkeypatch.setenv("TRACS_FILTER_LANES_MIN", lanes_min)
    for name, case in sorted(FILTER_CASES.items()):
        r, c, d, _, filt = PC.expected(ARRAYS, case)
        aln = _packed(case["aln"])
        got, found, pos, off = dev.filter_recomb_device(aln, *_dev(r, c, d))
        assert np.array_equal(found.cpu().numpy(), d), name
        assert np.array_equal(got.cpu().numpy(), filt), (name, np.nonzero(got.cpu().numpy() != filt)[0][:8])
        pos, off = pos.cpu().numpy(), off.cpu().numpy()
        assert all((np.diff(pos[off[t]:off[t + 1]]) > 0).all() for t in range(len(r)))
        aln.close()


@pytest.mark.parametrize("table", ["rows", "per-entry sum"])
def test_filter_recomb_lists_equals_the_reference_on_the_position_lists(hiplib, monkeypatch, table):
    """every position list of filter_hp_golden.json: what ref_filter_recomb_positions returned for it"""
    import json
    import torch
    import hp_filter as H
    from tracs_amd import device as dev
    if table != "rows":
        monkeypatch.setenv("TRACS_FILTER_TABLE", "0")
    with open(os.path.join(HERE, "golden", "filter_hp_golden.json")) as fh:
        lists = PC.hp_lists(H, json.load(fh)["cases"])
    want = ARRAYS["hp/ref"].reshape(-1)
    assert len(lists) == len(want) == META["hp_lists"]
    for L in sorted({x[0] for x in lists}):
        mine = [t for t, x in enumerate(lists) if x[0] == L]
        aln = dev.Alignment(1, L)
        aln.pack(np.full((1, L), ord("A"), np.uint8))
        off = np.zeros(len(mine) + 1, np.int64)
        off[1:] = np.cumsum([len(lists[t][2]) for t in mine])
        pos = np.concatenate([lists[t][2] for t in mine]).astype(np.int32)
        filt, _ = dev.filter_recomb_lists(aln, torch.from_numpy(off).cuda(), torch.from_numpy(pos).cuda(), with_dropped=False)
        got = filt.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want[mine]), (table, L, np.nonzero(got != want[mine])[0][:8])
        aln.close()


@pytest.mark.parametrize("name", sorted(FILTER_CASES))
def test_pairsnp_with_filter_from_fasta_equals_the_reference(hiplib, tmp_path, name):
    """end to end: the six columns of pairsnp(filter = True), thresholded or not"""
    want = _api_case(FILTER_CASES[name], tmp_path)
    assert (want[4] < want[2]).any()
