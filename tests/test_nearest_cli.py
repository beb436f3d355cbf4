"""`tracs distance --nearest K` on the host: the flag's default and bounds, and the refusal of --gpus N > 1 before any GPU call."""
import argparse
import os

import pytest


def _parser():
    from tracs_amd.distance import distance_parser
    return distance_parser(argparse.ArgumentParser())


def test_nearest_default_off():
    a = _parser().parse_args(["--msa", "x.fa", "-o", "o.csv"])
    assert a.nearest is None


@pytest.mark.parametrize("k", ["1", "10", "1024"])
def test_nearest_accepts_bounds(k):
    assert _parser().parse_args(["--msa", "x.fa", "-o", "o.csv", "--nearest", k]).nearest == int(k)


@pytest.mark.parametrize("k", ["0", "-1", "1025"])
def test_nearest_rejects_out_of_range(k, capsys):
    with pytest.raises(SystemExit) as e:
        _parser().parse_args(["--msa", "x.fa", "-o", "o.csv", "--nearest", k])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "argument --nearest" in err and "K must be in [1, 1024]" in err


def test_nearest_rejects_non_integer(capsys):
    with pytest.raises(SystemExit) as e:
        _parser().parse_args(["--msa", "x.fa", "-o", "o.csv", "--nearest", "x"])
    assert e.value.code == 2
    assert "argument --nearest: invalid check_nearest_k value: 'x'" in capsys.readouterr().err


def test_nearest_refuses_several_gpus(tmp_path, monkeypatch):
    import tracs_amd.distance as di
    from tracs_amd import multigpu

    def no_gpu(*a, **k):
        raise AssertionError("a GPU path was entered")
    monkeypatch.setattr(multigpu, "spawn", no_gpu)
    monkeypatch.setattr(multigpu, "init", no_gpu)
    monkeypatch.setattr(di, "nearest_arrays", no_gpu)
    monkeypatch.setattr(di, "pairsnp_arrays", no_gpu)
    out = tmp_path / "o.csv"
    a = _parser().parse_args(["--msa", "x.fa", "-o", str(out), "--nearest", "3", "--gpus", "2"])
    with pytest.raises(SystemExit) as e:
        a.func(a)
    assert "--nearest" in str(e.value.code) and "--gpus" in str(e.value.code)
    assert not os.path.exists(out)


def test_nearest_takes_the_array_route(tmp_path, monkeypatch, oracle):
    """With --nearest the CLI asks nearest_arrays (here: the oracle's all-pairs lists cut to K) and writes its rows."""
    import numpy as np

    import tracs_amd.distance as di
    from tracs_amd import synth
    seqs = synth.alignment(12, 300, seed=3, mu_lineage=2e-2, mu_sample=1e-2, p_n=0.02)
    fa = tmp_path / "aln_combined.fasta"
    synth.write_fasta(str(fa), seqs)
    seen = {}

    def nearest_arrays(fasta, k, n_threads=1, dist=2147483647, filter=False):
        seen.update(fasta=fasta, k=k, dist=dist, filter=filter)
        r, c, d, nn = oracle.pairsnp_arrays(seqs)
        rows, cols = np.concatenate([r, c]), np.concatenate([c, r])
        d, nn = np.concatenate([d, d]), np.concatenate([nn, nn])
        o = np.lexsort((cols, d, rows))
        rows, cols, d, nn = rows[o], cols[o], d[o], nn[o]
        first = np.searchsorted(rows, rows)
        keep = np.arange(len(rows)) - first < k
        return rows[keep], cols[keep], d[keep], ["s%d" % i for i in range(12)], np.zeros(int(keep.sum()), np.uint64), nn[keep]

    def refuse(*a, **kw):
        raise AssertionError("--nearest must not take the all-pairs route")
    monkeypatch.setattr(di, "nearest_arrays", nearest_arrays)
    monkeypatch.setattr(di, "pairsnp_arrays", refuse)
    monkeypatch.setattr(di, "_rows_on_device", refuse)
    out = tmp_path / "o.csv"
    a = _parser().parse_args(["--msa", str(fa), "-o", str(out), "--nearest", "2", "-D", "40", "--loglevel", "ERROR"])
    a.func(a)
    assert seen["k"] == 2 and seen["dist"] == 40 and seen["filter"] is False
    lines = out.read_text().strip().split("\n")
    assert lines[0] == di.HEADER.strip()
    assert len(lines) == 1 + 12 * 2
    firsts = [ln.split(",")[0] for ln in lines[1:]]
    assert all(firsts.count("s%d" % i) == 2 for i in range(12))
