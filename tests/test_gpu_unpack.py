"""Planes back to text (csrc/msa_out.hip: unpack_kernel): every byte of the canonical text against lut[mask_table[seqs]], what the
kernel must NOT write (beyond column L, outside the sample range), the round trip through the pack byte for byte, the errors."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LUT = np.frombuffer(b"XACMGRSVTWYHKDBN", np.uint8)
SHAPES = [(5, 1), (33, 129), (64, 128), (65, 4097), (131, 30001)]
FILL = 0xEE


def _mask_table(hiplib):
    return np.array([hiplib.tracs_debug_iupac_mask(ch) for ch in range(256)], np.uint8)


def _input(n, L):
    from tracs_amd import synth
    seqs = synth.alignment(n, L, seed=n * 7 + L, mu_lineage=3e-2, mu_sample=1e-2, p_n=0.05, p_partial=0.05, p_lower=0.05, p_other=0.03)
    rng = np.random.default_rng(n + L)
    for byte in (ord("-"), 0x07, 0xC3):                     # '-', a byte below 0x20, one above 0x7F: all N
        seqs[rng.integers(0, n), rng.integers(0, L)] = byte
    seqs[n - 1, L - 1] = 0x9F                               # ... and in the last valid site of the last group, last sample
    seqs[0, 0] = ord("-")
    return seqs


def _packed(seqs):
    from tracs_amd import device as dev
    a = dev.Alignment(*seqs.shape)
    a.pack(np.ascontiguousarray(seqs))
    return a


def _plane_bytes(aln):
    import torch
    from tracs_amd.multigpu import _DeviceBytes
    torch.cuda.synchronize()
    return torch.as_tensor(_DeviceBytes(aln.planes_ptr(), aln.nbytes), device="cuda").cpu().numpy().copy()


def make_case(n, L, hiplib):
    """one alignment of the module's shapes, packed, with what the tests compare against (a generator: closes the handle at the end;
    tests/test_gpu_scratch_poison.py builds the same cases per test)"""
    seqs = _input(n, L)
    table = _mask_table(hiplib)
    assert (table[seqs] != 0).all() and table[ord("-")] == 15 and table[0x07] == 15 and table[0xC3] == 15 and table[ord("r")] == 5
    src = _packed(seqs)
    yield dict(n=n, L=L, seqs=seqs, expect=LUT[table[seqs]], src=src, before=_plane_bytes(src))
    src.close()


@pytest.fixture(scope="module", params=SHAPES, ids=["%dx%d" % s for s in SHAPES])
def case(request, hiplib):
    yield from make_case(*request.param, hiplib)


def _ranges(n):
    out = [(0, n)]
    if n >= 3:
        out.append((1, n - 2))
    if n >= 65:
        out.append((63, 2))                                 # crosses a 64-sample block
    return out


@pytest.mark.parametrize("extra", [0, 13], ids=["stride=L", "stride=L+13"])
def test_text_and_what_stays_untouched(case, extra):
    import torch
    n, L, src, expect = case["n"], case["L"], case["src"], case["expect"]
    stride = L + extra
    if L > 1:
        assert (expect != case["seqs"]).any()              # lower case, '-', other bytes: canonical text is not the input
    for first, count in _ranges(n):
        # rows [0, n) of a buffer of n + 2 rows; the call writes rows [first, first + count) of the view that starts one row in
        buf = torch.full((n + 2, stride), FILL, dtype=torch.uint8, device="cuda")
        view = buf[1 + first:1 + first + count]
        got = src.unpack(first=first, count=count, stride=stride, out=view)
        torch.cuda.synchronize()
        assert got.data_ptr() == view.data_ptr()
        host = buf.cpu().numpy()
        rows = host[1 + first:1 + first + count]
        assert np.array_equal(rows[:, :L], expect[first:first + count]), (first, count)
        assert (rows[:, L:] == FILL).all(), (first, count)                       # no byte at or beyond column L
        assert (host[:1 + first] == FILL).all() and (host[1 + first + count:] == FILL).all(), (first, count)       # no other row
    assert np.array_equal(_plane_bytes(src), case["before"])                    # the source is left as it was


def test_default_arguments(case):
    n, L, src = case["n"], case["L"], case["src"]
    got = src.unpack()
    assert tuple(got.shape) == (n, L) and np.array_equal(got.cpu().numpy(), case["expect"])
    if n > 2:
        got = src.unpack(first=2)
        assert tuple(got.shape) == (n - 2, L) and np.array_equal(got.cpu().numpy(), case["expect"][2:])


def test_round_trip_byte_for_byte(case):
    """packing the canonical text gives the source's bytes back: all nbytes, pads and slack included"""
    from tracs_amd import device as dev
    n, L, src = case["n"], case["L"], case["src"]
    text = src.unpack()
    twin = dev.Alignment(n, L)
    twin.pack(text)                                         # (device to device)
    assert twin.nbytes == src.nbytes
    a = _plane_bytes(twin)
    assert np.array_equal(a, case["before"]), int((a != case["before"]).sum())
    twin.close()
    assert np.array_equal(_plane_bytes(src), case["before"])


def test_argument_errors_leave_the_buffer_alone(hiplib):
    import ctypes as C

    import torch
    seqs = _input(33, 129)
    src = _packed(seqs)
    buf = torch.full((40, 140), FILL, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError) as e:
        src.unpack(first=30, count=4, stride=140, out=buf)                       # first + count > n
    assert "sample range" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        src.unpack(first=0, count=33, stride=128, out=buf)                       # stride < L
    assert "stride" in str(e.value)
    rc = hiplib.tracs_alignment_unpack(src._h, 0, 33, None, 140, None)           # a NULL pointer
    assert rc == -1 and b"NULL" in hiplib.tracs_last_error()
    rc = hiplib.tracs_alignment_unpack(None, 0, 33, C.c_void_p(buf.data_ptr()), 140, None)
    assert rc == -1 and b"NULL" in hiplib.tracs_last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == FILL).all()
    src.close()
