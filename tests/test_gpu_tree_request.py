"""tracs_distance_tree_run against the five older entry points on the GPU (include/tracs_hip.h): the same handle, the
equivalent request, two folders -- every file byte for byte, the result against the older call's out-parameters, and the two refusals
that only a request can spell.  n = 1, 2: nothing runs on the device; 3: no join; 4: the first internal edge; 5: more than one join;
67: past one wave of 64 lanes and one pad of samples.  L = 300: two full groups of 128 sites and a tail."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 4, 5, 67]
L = 300
FILES = ("path", "edges_path", "replicate_trees_path", "changes_path", "sites_path", "filtered_path")
COUNTERS = ("n_joins", "rows_written", "n_changes", "sum_minimum", "n_kept", "n_edges_dropped")
# kind of request -> (the request's fields beside kind, path, ref; the older entry point; the counters it returns)
BOOT = dict(replicates=3, seed=7, replicate_trees_path="reps.nwk")
ROWS = dict(changes=1, changes_path="c.csv", sites_path="s.csv", max_entries=100000000, n_threads=2)
KINDS = {"snp": (dict(kind=0), "tracs_distance_tree", 2),
         "per-site": (dict(kind=1), "tracs_distance_tree", 2),
         "bootstrap": (BOOT, "tracs_distance_tree_bootstrap", 2),
         "transfer": (dict(BOOT, transfer=1), "tracs_distance_tree_bootstrap_transfer", 2),
         "changes": (ROWS, "tracs_distance_tree_changes", 4),
         "filter": (dict(ROWS, filter=1, filtered_path="f.nwk"), "tracs_distance_tree_filter", 6)}


@pytest.fixture(scope="module")
def handles(tmp_path_factory, hiplib):
    """n -> an opened handle on a seeded random alignment of n samples with some N"""
    from tracs_amd.handle import DistanceHandle
    d = tmp_path_factory.mktemp("tree_request")
    rng = np.random.default_rng(20241119)
    opened = {}
    for n in NS:
        root = rng.choice(np.frombuffer(b"ACGT", np.uint8), L)
        seqs = np.where(rng.random((n, L)) < 0.2, rng.choice(np.frombuffer(b"ACGT", np.uint8), (n, L)), root)
        seqs[rng.random((n, L)) < 0.05] = ord("N")
        fa = d / ("n%d_combined.fasta" % n)
        fa.write_bytes(b"".join(b">s%d\n%s\n" % (i, seqs[i].astype(np.uint8).tobytes()) for i in range(n)))
        opened[n] = DistanceHandle([str(fa)])
    yield opened
    for h in opened.values():
        h.close()


def _request(folder, fields, create):
    from tracs_amd import _lib
    own = {k: os.fsencode(str(folder / v)) if k in FILES else v for k, v in fields.items()}
    return _lib.TreeRequest(**dict(dict(kind=0, path=os.fsencode(str(folder / "t.nwk")), ref=b"ref1", edges_path=os.fsencode(str(folder / "e.csv")),
                                        create=create), **own))


def _older(hiplib, entry, h, q, n_counters):
    """the older entry point on the request's own fields -> (return code, its out-parameters)"""
    out = [C.c_uint64(99) for _ in range(n_counters)]
    refs = [C.byref(x) for x in out]
    head = (h.h, q.kind, q.path, q.ref, q.edges_path)
    rows = (q.contig_names, q.contig_lengths, q.n_contigs, q.max_entries, q.n_threads, q.create)
    if entry == "tracs_distance_tree":
        rc = hiplib.tracs_distance_tree(*head, *refs)
    elif entry == "tracs_distance_tree_changes":
        rc = hiplib.tracs_distance_tree_changes(*head, q.changes_path, q.sites_path, *rows, *refs)
    elif entry == "tracs_distance_tree_filter":
        rc = hiplib.tracs_distance_tree_filter(*head, q.changes_path, q.sites_path, q.filtered_path, *rows, *refs)
    else:
        rc = getattr(hiplib, entry)(*head, q.replicates, q.seed, q.replicate_trees_path, *refs)
    return rc, [x.value for x in out]


def _files(folder):
    return {p.name: p.read_bytes() for p in sorted(folder.iterdir())}


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", NS)
def test_the_request_writes_what_the_older_entry_point_writes(hiplib, handles, tmp_path, n, kind):
    from tracs_amd import _lib
    fields, entry, n_counters = KINDS[kind]
    old_dir, new_dir = tmp_path / "older", tmp_path / "request"
    old_dir.mkdir()
    new_dir.mkdir()
    passes = (1, 0) if n in (NS[0], 5) else (1,)                # create = 0: a second --msa file of a run, the files are appended to
    for create in passes:
        rc, want = _older(hiplib, entry, handles[n], _request(old_dir, fields, create), n_counters)
        assert rc == 0, hiplib.tracs_last_error()
        res = _lib.TreeResult(*[99] * 6)
        rc = hiplib.tracs_distance_tree_run(handles[n].h, C.byref(_request(new_dir, fields, create)), C.byref(res))
        assert rc == 0, hiplib.tracs_last_error()
        assert [getattr(res, name) for name in COUNTERS] == want + [0] * (6 - n_counters)
        assert res.n_joins == max(n - 3, 0) and res.rows_written == (2 * n - 3 if n >= 3 else n - 1)
        got, older = _files(new_dir), _files(old_dir)
        assert sorted(got) == sorted(older) and got == older
    produced = {"t.nwk", "e.csv"} | {v for k, v in fields.items() if k in FILES}
    if "replicate_trees_path" in fields and n < 4:              # (no replicate is drawn where no edge can be labelled)
        produced.discard("reps.nwk")
    assert set(got) == produced
    assert got["t.nwk"].count(b"\n") == len(passes)


def test_what_only_a_request_can_ask_is_refused_and_touches_no_file(hiplib, handles, tmp_path):
    from tracs_amd import _lib
    for fields, words in ((dict(BOOT, **ROWS), b"cannot be combined yet"), (dict(BOOT, kind=1), b"SNP distance (kind 0) only"),
                          (dict(BOOT, transfer=1, **dict(ROWS, filter=1)), b"cannot be combined yet")):
        res = _lib.TreeResult(*[99] * 6)
        assert hiplib.tracs_distance_tree_run(handles[5].h, C.byref(_request(tmp_path, fields, 1)), C.byref(res)) == -1
        msg = hiplib.tracs_last_error()
        assert msg.startswith(b"tracs_distance_tree_run: ") and words in msg, msg
        assert [getattr(res, name) for name in COUNTERS] == [0] * 6
        assert list(tmp_path.iterdir()) == []
