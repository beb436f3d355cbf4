"""The host side of --msa-out / --site-table: the FASTA row writer, the differs table against its definition, and
the command line's refusals -- which come before anything touches the GPU, so none of this needs one."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write(hiplib, path, names, rows, L, append=0, threads=3, level=6):
    """rows: uint8 [count, stride]"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    count, stride = rows.shape
    arr = (C.c_char_p * max(count, 1))(*[x.encode() for x in names])
    return hiplib.tracs_write_fasta_rows(os.fsencode(path), arr, C.c_void_p(rows.ctypes.data), stride, count, L, append, threads, level)


def _rows(count, L, stride, seed):
    rng = np.random.default_rng(seed)
    rows = np.full((count, stride), 0xEE, np.uint8)                     # what lies beyond column L must never reach the file
    rows[:, :L] = np.frombuffer(b"ACGTNRYKM", np.uint8)[rng.integers(0, 9, (count, L))]
    return rows


def _expect(names, rows, L):
    return b"".join(b">" + nm.encode() + b"\n" + rows[k, :L].tobytes() + b"\n" for k, nm in enumerate(names))


def _gzip_members(data):
    """the lengths of the members of a gzip file, each inflated on its own"""
    import zlib
    out = []
    while data:
        d = zlib.decompressobj(16 + zlib.MAX_WBITS)
        out.append(d.decompress(data))
        assert d.eof
        data = d.unused_data
    return out


@pytest.mark.parametrize("suffix", [".fasta", ".fasta.gz"])
def test_writer_rows_stride_append(hiplib, tmp_path, suffix):
    L, stride = 1237, 1237 + 19
    names = ["s%d some text" % k for k in range(7)]
    rows = _rows(7, L, stride, 5)
    path = str(tmp_path / ("rows" + suffix))
    assert _write(hiplib, path, names[:4], rows[:4], L) == 0
    raw = open(path, "rb").read()
    first = gzip.decompress(raw) if suffix.endswith(".gz") else raw
    assert first == _expect(names[:4], rows[:4], L)
    assert _write(hiplib, path, names[4:], rows[4:], L, append=1) == 0
    raw = open(path, "rb").read()
    if suffix.endswith(".gz"):
        members = _gzip_members(raw)
        assert len(members) == 7                                         # one member per record ...
        assert members == [_expect([nm], rows[k:k + 1], L) for k, nm in enumerate(names)]
        with gzip.open(path, "rb") as fh:                                # ... and one stream to every reader
            assert fh.read() == _expect(names, rows, L)
    else:
        assert raw == _expect(names, rows, L) and b"\xee" not in raw
    # a call without append starts over
    assert _write(hiplib, path, names[:1], rows[:1], L) == 0
    raw = open(path, "rb").read()
    assert (gzip.decompress(raw) if suffix.endswith(".gz") else raw) == _expect(names[:1], rows[:1], L)


@pytest.mark.parametrize("suffix", [".fasta", ".fasta.gz"])
def test_writer_no_rows_and_errors(hiplib, tmp_path, suffix):
    path = str(tmp_path / ("empty" + suffix))
    with open(path, "wb") as fh:
        fh.write(b"stale")
    assert _write(hiplib, path, [], np.zeros((0, 8), np.uint8), 5) == 0
    assert os.path.getsize(path) == 0                                    # count = 0: an empty file
    rows = _rows(2, 10, 10, 1)
    assert _write(hiplib, path, ["a", "b"], rows, 10) == 0
    size = os.path.getsize(path)
    assert _write(hiplib, path, [], np.zeros((0, 8), np.uint8), 5, append=1) == 0 and os.path.getsize(path) == size
    bad = str(tmp_path / "no_such_folder" / ("x" + suffix))
    assert _write(hiplib, bad, ["a", "b"], rows, 10) == -5 and b"cannot open" in hiplib.tracs_last_error()
    assert _write(hiplib, path, ["a", "b"], rows, 11) == -1              # stride < L
    assert hiplib.tracs_write_fasta_rows(None, None, None, 0, 0, 0, 0, 1, 6) == -1


def test_differs_table_is_the_definition(hiplib):
    """bit p of the table, p = presence word (bit m - 1: mask m occurs, m = 1 .. 14): two present masks with an empty intersection"""
    raw = np.zeros(2048, np.uint8)
    assert hiplib.tracs_debug_differs_table(C.c_void_p(raw.ctypes.data), 2048) == 0
    got = np.unpackbits(raw, bitorder="little").astype(bool)
    assert got.shape == (1 << 14,)
    disjoint = [[a & b == 0 for b in range(1, 15)] for a in range(1, 15)]
    expect = np.zeros(1 << 14, bool)
    for p in range(1 << 14):
        present = [m for m in range(14) if (p >> m) & 1]
        expect[p] = any(disjoint[a][b] for i, a in enumerate(present) for b in present[i + 1:])
    assert np.array_equal(got, expect)
    bit = lambda *masks: sum(1 << (m - 1) for m in masks)               # noqa: E731
    assert not got[0] and not got[bit(1)] and not got[bit(5, 1)]         # R and A overlap
    assert got[bit(5, 2)] and got[bit(5, 10)] and got[bit(3, 12)] and got[bit(7, 8)] and got[bit(1, 4)]
    assert 0 < got.sum() < (1 << 14)
    assert hiplib.tracs_debug_differs_table(C.c_void_p(raw.ctypes.data), 100) == -1


def _cli(argv):
    return subprocess.run([sys.executable, "-m", "tracs_amd", "distance"] + argv, capture_output=True, text=True, timeout=120, cwd=ROOT)


REFUSALS = {
    "msa-db": (["--msa", "A", "--msa-db", "B", "--msa-out", "OUT"], "take no --msa-db"),
    "msa-db with the table": (["--msa", "A", "--msa-db", "B", "--site-table", "TAB"], "take no --msa-db"),
    "two msa files": (["--msa", "A", "B", "--msa-out", "OUT"], "give one --msa file"),
    "two msa files with the table": (["--msa", "A", "B", "--site-table", "TAB"], "give one --msa file"),
    "gpus": (["--msa", "A", "--gpus", "2", "--msa-out", "OUT"], "run on one GPU"),
    "gpus with the table": (["--msa", "A", "--gpus", "2", "--site-table", "TAB"], "run on one GPU"),
    "msa-out-sites alone": (["--msa", "A", "--msa-out-sites", "differing"], "--msa-out-sites needs --msa-out"),
    "msa-out-sites with the table alone": (["--msa", "A", "--msa-out-sites", "kept", "--site-table", "TAB"], "--msa-out-sites needs --msa-out"),
    "output is the input": (["--msa", "A", "--msa-out", "A"], "is one of the run's input files"),
    "table is the metadata": (["--msa", "A", "--meta", "META", "--site-table", "META"], "is one of the run's input files"),
    "output is the mask": (["--msa", "A", "--mask", "BED", "--msa-out", "BED"], "is one of the run's input files"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_cli_refusals(tmp_path, case):
    """each refusal exits non-zero with its message and before the library is asked for anything: the inputs hold what would make
    the run itself fail differently (a FASTA that is none), and nothing is written"""
    files = {"A": str(tmp_path / "a_combined.fasta"), "B": str(tmp_path / "b.fasta"), "META": str(tmp_path / "meta.csv"),
             "BED": str(tmp_path / "mask.bed"), "OUT": str(tmp_path / "out.fasta"), "TAB": str(tmp_path / "table.csv")}
    for k in ("A", "B", "META", "BED"):
        with open(files[k], "w") as fh:
            fh.write("not what it should be\n")
    argv, message = REFUSALS[case]
    csv = str(tmp_path / "out.csv")
    p = _cli([files.get(x, x) for x in argv] + ["-o", csv])
    assert p.returncode != 0 and message in p.stderr, p.stderr[-2000:]
    assert p.stderr.strip().startswith("tracs distance:") and "Traceback" not in p.stderr
    assert not os.path.exists(csv) and not os.path.exists(files["OUT"]) and not os.path.exists(files["TAB"])
    assert open(files["A"]).read() == "not what it should be\n"
