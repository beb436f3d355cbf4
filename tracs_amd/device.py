"""Device-resident entry points (include/tracs_hip.h part 2) over torch tensors.

torch is used for device memory, streams and torch.distributed only -- plumbing; every kernel is
in libtracs_hip.so.  Import torch BEFORE this module's first call so that both share one HIP
runtime (torch ships its own libamdhip64.so with the same soname).
"""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _panel_ptr(t, base_row):
    """Pointer the dense entry points can index with ABSOLUTE row numbers when `t` ([rows, ld]) only holds rows
    base_row.. of the matrix (row panels of matrices too large to allocate whole)."""
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr() - int(base_row) * t.stride(0) * t.element_size())


class Alignment:
    """A packed alignment resident in HBM (tracs_alignment)."""

    def __init__(self, n, L):
        self._L = _lib.require_gpu()
        self._h = C.c_void_p()
        _lib.check(self._L.tracs_alignment_create(int(n), int(L), C.byref(self._h)))
        self.n, self.L = int(n), int(L)

    @classmethod
    def from_fasta(cls, paths):
        import os
        L = _lib.require_gpu()
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        h, names, nb, n0 = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
        _lib.check(L.tracs_alignment_from_fasta(arr, len(paths), C.byref(h), C.byref(names), C.byref(nb), C.byref(n0)))
        self = cls.__new__(cls)
        self._L, self._h = L, h
        self.n, self.L = L.tracs_alignment_n(h), L.tracs_alignment_len(h)
        raw = C.string_at(names, nb.value) if nb.value else b""
        L.tracs_free(names)
        self.names = [x.decode("utf-8", "replace") for x in raw.split(b"\0")[:self.n]]
        self.n_first = n0.value
        return self

    @classmethod
    def borrowed(cls, lib, handle):
        """A view of a tracs_alignment that another handle owns (tracs_distance_alignment): close() and __del__ leave it alone."""
        self = cls.__new__(cls)
        self._L, self._h, self._borrowed = lib, C.c_void_p(handle), True
        self.n, self.L = lib.tracs_alignment_n(self._h), lib.tracs_alignment_len(self._h)
        return self

    def pack(self, ascii_u8, first=0):
        """ascii_u8: torch.uint8 [count, L] on the GPU, or a numpy uint8 array on the host."""
        if isinstance(ascii_u8, torch.Tensor):
            assert ascii_u8.dtype == torch.uint8 and ascii_u8.is_contiguous() and ascii_u8.shape[1] == self.L
            on_dev = 1 if ascii_u8.is_cuda else 0
            ptr, count = C.c_void_p(ascii_u8.data_ptr()), ascii_u8.shape[0]
        else:
            a = np.ascontiguousarray(ascii_u8, dtype=np.uint8)
            assert a.ndim == 2 and a.shape[1] == self.L
            on_dev, ptr, count = 0, C.c_void_p(a.ctypes.data), a.shape[0]
        _lib.check(self._L.tracs_alignment_pack(self._h, ptr, int(first), int(count), on_dev, _stream()))

    def mark_packed(self):
        """The planes were written from outside the library (a broadcast from another rank): drop every cached derived form."""
        _lib.check(self._L.tracs_alignment_touch(self._h))

    def hint_rows(self, ranges):
        """A multi-GPU rank's promise: this handle will only be asked for rows inside `ranges` ([(begin, end), ..], at most two;
        [] lifts it), so what is built per row once per pack is built for those rows only.  Dense calls for other rows fail."""
        flat = [int(x) for r in ranges for x in r]
        arr = (C.c_size_t * max(len(flat), 1))(*flat)
        _lib.check(self._L.tracs_alignment_hint_rows(self._h, arr, len(ranges)))

    def pack_codes(self, codes, sample):
        """Pack samples straight from their packed 4-bit allele masks (posterior_codes_device output):
        codes uint8 [(L+1)//2] -> one sample, or uint8 [count, stride >= (L+1)//2] -> samples sample..sample+count-1."""
        assert codes.dtype == torch.uint8 and codes.is_cuda
        if codes.dim() == 1:
            assert codes.numel() == (self.L + 1) // 2
            _lib.check(self._L.tracs_alignment_pack_codes(self._h, _ptr(codes), int(sample), _stream()))
        else:
            assert codes.dim() == 2 and codes.stride(1) == 1 and codes.shape[1] >= (self.L + 1) // 2
            _lib.check(self._L.tracs_alignment_pack_codes_batch(self._h, _ptr(codes), int(codes.stride(0)), int(sample),
                                                                int(codes.shape[0]), _stream()))

    @property
    def encoding(self):
        """'consensus' (3 planes) / 'general' (5 planes) as used by the last dense call, None before the first."""
        e = self._L.tracs_debug_alignment_encoding(self._h)
        return {0: "general", 1: "consensus"}.get(e)

    @property
    def kernel(self):
        """'mfma' (matrix-core kernel, consensus operands) / 'mfma-general' (matrix-core kernel, one-hot operands + sparse
        partial-code correction) / 'valu' (tile kernel) as used by the last dense call, None before the first."""
        return {0: "valu", 1: "mfma", 2: "mfma-general"}.get(self._L.tracs_debug_alignment_kernel(self._h))

    @property
    def site_classes(self):
        """(dense, counted, minority, full) sites when the last dense call ran on site classes (csrc/site_classes.hip): the
        pair kernel read the dense sites only, a one-operand pass over the counted sites (and a constant for the full ones:
        nobody is N there) completed the compared-sites counts, and the minority sites -- counted or full sites at which a few
        samples differ -- added their distances from sparse lists; None when the whole alignment was read."""
        import ctypes as C
        out = (C.c_uint64 * 4)()
        state = self._L.tracs_debug_alignment_site_classes(self._h, out)
        return tuple(int(x) for x in out) if state == 1 else None

    @property
    def nw_gram(self):
        """True when the minority sites' N x listed terms of the last decided classes come from two one-plane passes on the matrix cores
        (U U^T - n n^T, csrc/site_classes.hip) instead of walks of the sites' N lists."""
        return bool(self._L.tracs_debug_alignment_nw_gram(self._h))

    @property
    def nw_form(self):
        """None / 'u-pass' (U U^T - n n^T: two one-plane matrix passes) / 'ns-rows' (the rows of the site-major N matrix summed per listed
        sample inside the fix-up: one matrix pass, for the compared sites alone) -- how the second form of the classes gets its terms."""
        return {0: None, 1: "u-pass", 2: "ns-rows"}.get(self._L.tracs_debug_alignment_nw_gram(self._h))

    @property
    def count_source(self):
        """(sites the counting pass reads on the matrix cores, in_place, sites whose N co-occurrences come from lists) for an
        alignment on site classes: in_place = the stored N plane of every site, read where it lies (the pair kernels then write d
        only); else the N plane of the sites with many N samples, re-packed.  None without classes."""
        out = (C.c_uint64 * 8)()
        return (int(out[0]), bool(out[1]), int(out[2])) if self._L.tracs_debug_alignment_count_source(self._h, out) else None

    @property
    def list_stats(self):
        """{nn_visits, nn_walks, n_lines, p_entries, n_entry_bytes[, max_row_n, bitmaps, row_splits, row_lists, row_list_lines]}: list entries one pass of the N
        co-occurrence walk decodes (sum of cN^2 over the sites whose co-occurrences come from lists) in how many list walks (sum of
        cN), 128-byte lines reserved for the per-site N lists, entries of the listed-sample lists, bytes per N list entry; the most N
        sites any sample has and the workgroups its row is cut over; None without classes."""
        out = (C.c_uint64 * 8)()
        if not self._L.tracs_debug_alignment_count_source(self._h, out):
            return None
        st = {"nn_visits": int(out[3]), "n_lines": int(out[4]), "p_entries": int(out[5]), "n_entry_bytes": int(out[6]),
              "nn_walks": int(out[7])}
        sizes = (C.c_uint64 * 8)()
        if self._L.tracs_debug_lists(self._h, 0, sizes, 64) == 64:
            # (nn_rows_kernel cuts a row over up to 32 workgroups by its N sites: csrc/site_lists.hip)
            target = max(8192, st["nn_walks"] // 2048)
            st.update(max_row_n=int(sizes[7]), bitmaps=bool(sizes[5]), row_splits=min(32, max(1, -(-int(sizes[7]) // target))))
            # (the rows' N sites as slots of 16-bit entries instead of bitmaps, and the 128-byte lines of them that the build wrote)
            rl = (C.c_uint64 * 2)()
            has = self._L.tracs_debug_lists(self._h, 13, rl, 16) == 16
            st.update(row_lists=bool(has and rl[0]), row_list_lines=int(rl[1]) if has else 0)
        return st

    def site_n_counts(self):
        """torch.int32 [L] on the device: per site, the samples that are N there (the stored N plane: 'N', '-' and every byte that
        is not an IUPAC letter; partial codes are not N).  tracs_alignment_site_n_counts."""
        out = torch.empty(self.L, dtype=torch.int32, device="cuda")
        _lib.check(self._L.tracs_alignment_site_n_counts(self._h, _ptr(out), _stream()))
        return out

    def select_sites(self, keep=None, max_n_samples=None):
        """-> (Alignment over the kept columns, kept bool ndarray [L]): a column stays when keep (bool per column; None: all) allows
        it and at most max_n_samples samples are N there (None: no rule).  The new handle is byte for byte what packing the
        column-deleted sequences gives; this one is left as it was.  tracs_alignment_select_sites."""
        from .sites import Sites, bitmap_to_bool
        words, keep_len, max_n = Sites(keep, max_n_samples).c_args()
        kept = np.zeros((self.L + 63) // 64, np.uint64)
        h, n_kept = C.c_void_p(), C.c_size_t(0)
        u64p = C.POINTER(C.c_uint64)
        _lib.check(self._L.tracs_alignment_select_sites(self._h, words.ctypes.data_as(u64p) if words is not None else None, keep_len, max_n,
                                                        C.byref(h), kept.ctypes.data_as(u64p), C.byref(n_kept), _stream()))
        new = Alignment.__new__(Alignment)
        new._L, new._h = self._L, h
        new.n, new.L = self.n, int(n_kept.value)
        for attr in ("names", "n_first"):
            if hasattr(self, attr):
                setattr(new, attr, getattr(self, attr))
        return new, bitmap_to_bool(kept, self.L)

    def sample_n_counts(self, keep=None):
        """torch.int32 [n] on the device: per sample, the sites at which it is N (the stored N plane, as site_n_counts) among the
        columns keep (bool per column; None: all) leaves.  tracs_alignment_sample_n_counts."""
        from .sites import Sites
        words, keep_len, _ = Sites(keep).c_args()
        out = torch.empty(self.n, dtype=torch.int32, device="cuda")
        _lib.check(self._L.tracs_alignment_sample_n_counts(self._h, words.ctypes.data_as(C.POINTER(C.c_uint64)) if words is not None else None,
                                                           keep_len, _ptr(out), _stream()))
        return out

    def select_samples(self, mask):
        """-> Alignment over the samples mask (one bool per sample) keeps, in their order: byte for byte what packing the kept
        sequences gives; this one is left as it was.  tracs_alignment_select_samples."""
        m = np.ascontiguousarray(np.asarray(mask, dtype=bool).astype(np.uint8))
        if m.ndim != 1 or m.shape[0] != self.n:
            raise ValueError("select_samples: the mask covers %s samples, the alignment has %d" % (m.shape[0] if m.ndim == 1 else m.shape, self.n))
        h = C.c_void_p()
        _lib.check(self._L.tracs_alignment_select_samples(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(h), _stream()))
        new = Alignment.__new__(Alignment)
        new._L, new._h = self._L, h
        new.n, new.L = int(m.sum()), self.L
        if hasattr(self, "names"):
            new.names = [x for x, k in zip(self.names, m) if k]
        if hasattr(self, "n_first"):
            new.n_first = int(m[:self.n_first].sum())
        return new

    def site_census(self):
        """-> (torch.int32 [6, L] on the device, bool ndarray [L]): per site, the samples whose allele mask is exactly A, C, G, T, all
        four (N), or a partial code -- the six rows sum to n --, and whether the site differs: two samples with disjoint masks, the
        sites that add 1 to some SNP distance.  Pad samples never count.  tracs_alignment_site_census."""
        from .sites import bitmap_to_bool
        counts = torch.empty((6, self.L), dtype=torch.int32, device="cuda")
        words = np.zeros((self.L + 63) // 64, np.uint64)
        _lib.check(self._L.tracs_alignment_site_census(self._h, _ptr(counts), words.ctypes.data_as(C.POINTER(C.c_uint64)), None, _stream()))
        return counts, bitmap_to_bool(words, self.L)

    def unpack(self, first=0, count=None, stride=None, out=None):
        """-> torch.uint8 [count, stride] on the device: samples [first, first + count) as canonical text ("XACMGRSVTWYHKDBN"[mask];
        packing it gives this handle's bytes back).  Only the first L bytes of each row are written (stride: default L).  out: a
        contiguous uint8 device tensor [count, stride] to write into.  tracs_alignment_unpack."""
        count = self.n - int(first) if count is None else int(count)
        stride = self.L if stride is None else int(stride)
        if out is None:
            out = torch.empty((max(count, 0), stride), dtype=torch.uint8, device="cuda")
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.numel() >= max(count, 0) * stride
        _lib.check(self._L.tracs_alignment_unpack(self._h, int(first), count, _ptr(out), stride, _stream()))
        return out

    @property
    def nbytes(self):
        return self._L.tracs_alignment_bytes(self._h)

    def planes_ptr(self):
        return self._L.tracs_alignment_planes(self._h)

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self._L.tracs_alignment_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bootstrap_weights(L, seed, b):
    """torch.int32 [L] on the device (bit pattern uint32): how often bootstrap replicate b under `seed` draws each of L columns
    (DESIGN.md 3.18); the counts sum to L.  tracs_bootstrap_weights."""
    lib = _lib.require_gpu()
    out = torch.empty(int(L), dtype=torch.int32, device="cuda")
    _lib.check(lib.tracs_bootstrap_weights(int(L), int(seed), int(b), _ptr(out), _stream()))
    return out


def gather_sites(aln, weights):
    """-> Alignment in which column c of `aln` is repeated weights[c] times, columns in ascending c: byte for byte what packing that
    text gives; `aln` is left as it was.  weights: one non-negative integer per column (a device int32 / uint32 tensor is used where it
    lies, anything else is copied).  A sum of 0 or of 2^32 and more is refused.  tracs_alignment_gather_sites."""
    if isinstance(weights, torch.Tensor) and weights.is_cuda and weights.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)):
        w = weights.contiguous()
    else:
        host = np.ascontiguousarray(weights.cpu().numpy() if isinstance(weights, torch.Tensor) else weights)
        if host.size and (host.min() < 0 or host.max() > 0xFFFFFFFF):
            raise ValueError("gather_sites(): a weight outside [0, 2^32)")
        w = torch.from_numpy(host.astype(np.uint32).view(np.int32)).cuda()
    if w.dim() != 1 or w.numel() != aln.L:
        raise ValueError("gather_sites(): %d weights for an alignment of %d columns" % (w.numel(), aln.L))
    h, n_out = C.c_void_p(), C.c_size_t(0)
    _lib.check(aln._L.tracs_alignment_gather_sites(aln._h, _ptr(w), C.byref(h), C.byref(n_out), _stream()))
    new = Alignment.__new__(Alignment)
    new._L, new._h = aln._L, h
    new.n, new.L = aln.n, int(n_out.value)
    for attr in ("names", "n_first"):
        if hasattr(aln, attr):
            setattr(new, attr, getattr(aln, attr))
    return new


def notify_distances(event):
    """The next pairsnp_dense call records `event` (torch.cuda.Event) on its stream once the distances are final -- before the
    compared-sites counts are (include/tracs_hip.h, "Two streams")."""
    if not event.cuda_event:
        # torch creates the hipEvent lazily, on the first record: force it into existence (the handle of an unrecorded
        # torch.cuda.Event is 0 -- the library would then record nothing and a wait on the event would not wait)
        event.record(torch.cuda.current_stream())
    if not event.cuda_event:
        raise _lib.TracsError("notify_distances: the event has no HIP handle")
    _lib.load().tracs_pairsnp_notify_distances(C.c_void_p(event.cuda_event))


def set_stream_policy(caller_orders_streams):
    _lib.load().tracs_set_stream_policy(1 if caller_orders_streams else 0)


@contextlib.contextmanager
def poison_scratch(byte):
    """Tests: while inside, every outermost entry-point call first fills the device's scratch slots with `byte` (0 .. 255), and
    a slot that grows inside a call starts as `byte` (tracs_debug_poison_scratch).  Switched off on the way out."""
    if not 0 <= int(byte) <= 255:
        raise ValueError("poison_scratch: byte must be 0 .. 255")
    lib = _lib.load()
    lib.tracs_debug_poison_scratch(int(byte))
    try:
        yield
    finally:
        lib.tracs_debug_poison_scratch(-1)


def scratch_hits():
    """How often each scratch slot (csrc/common.h's WsSlot, in order) has been handed out since the previous call; the counts
    are reset (tracs_debug_scratch_hits)."""
    lib = _lib.load()
    hits = (C.c_uint64 * 1024)()          # (one call: reading the counts resets them)
    n = lib.tracs_debug_scratch_hits(hits, len(hits))
    assert n <= len(hits)
    return [int(x) for x in hits[:n]]


def alloc_stats():
    """(live device blocks, live device bytes, live pinned blocks, allocations since the previous call) of the library's
    allocation path; the fourth is reset (tracs_debug_alloc_stats)."""
    out = (C.c_uint64 * 4)()
    _lib.load().tracs_debug_alloc_stats(out)
    return tuple(int(x) for x in out)


def fail_alloc(nth):
    """Tests: the nth allocation from now (1-based, device or pinned) fails as out of memory, once; 0 switches it off
    (tracs_debug_fail_alloc)."""
    _lib.load().tracs_debug_fail_alloc(int(nth))


def pack_stages():
    """[(stage, ms), ..] of the last once-per-pack build (encoding decision, site classes, lists), from HIP events on the launch
    stream; recorded when tracs_debug_pack_timing(1) was set before the dense call (diagnostics: bench.py's single_pass)."""
    lib = _lib.load()
    names = C.create_string_buffer(1024)
    ms = (C.c_float * 16)()
    k = lib.tracs_debug_pack_stages(names, 1024, ms, 16)
    return list(zip(names.value.decode().split("\n"), [float(x) for x in ms[:k]])) if k else []


def pack_stages_bytes():
    """[(stage, ms, bytes read, bytes written), ..] of the last once-per-pack build: pack_stages() with the library's own
    accounting of what each stage reads and writes (bench.py's roofline_per_pack)."""
    lib = _lib.load()
    st = pack_stages()
    rd, wr = (C.c_double * 16)(), (C.c_double * 16)()
    k = lib.tracs_debug_pack_stage_bytes(rd, wr, 16)
    return [(name, ms, float(rd[i]) if i < k else 0.0, float(wr[i]) if i < k else 0.0) for i, (name, ms) in enumerate(st)]


def pairsnp_dense(aln, dist, ncomp=None, row_begin=0, row_end=None, col_begin=0, dist_threshold=None, base_row=0):
    """dist/ncomp: torch.int32 (bit pattern uint32) device matrices [rows, ld >= n] holding rows base_row.. of the pair matrix,
    written for the cells rows [row_begin,row_end) x cols [max(col_begin,i+1), n).  With dist_threshold, pairs beyond it may
    come back negative (bit 31 set) with an unspecified ncomp: tiles stop early once all their pairs are past the threshold."""
    row_end = aln.n if row_end is None else row_end
    ld = dist.stride(0)
    assert base_row <= row_begin and row_end - base_row <= dist.shape[0]
    if dist_threshold is None:
        _lib.check(aln._L.tracs_pairsnp_dense(aln._h, int(row_begin), int(row_end), int(col_begin), _panel_ptr(dist, base_row),
                                              _panel_ptr(ncomp, base_row), int(ld), _stream()))
    else:
        _lib.check(aln._L.tracs_pairsnp_dense_thr(aln._h, int(row_begin), int(row_end), int(col_begin), _panel_ptr(dist, base_row),
                                                  _panel_ptr(ncomp, base_row), int(ld), int(dist_threshold), _stream()))


def pairs_min_sites(dist, ncomp, n, min_sites, row_begin=0, row_end=None, col_begin=0, dist_threshold=2147483647, base_row=0):
    """The pair rule on a dense panel (dist / ncomp as pairsnp_dense wrote them), in place: every cell of rows [row_begin, row_end) x
    cols [max(col_begin, i + 1), n) that is within dist_threshold (read unsigned) and was compared over fewer than min_sites sites
    gets the distance 0xFFFFFFFF (-1), which every consumer reads as beyond the threshold.  tracs_pairs_min_sites."""
    L = _lib.require_gpu()
    row_end = n if row_end is None else row_end
    ld = dist.stride(0)
    assert ncomp.stride(0) == ld and base_row <= row_begin and row_end - base_row <= dist.shape[0]
    _lib.check(L.tracs_pairs_min_sites(_panel_ptr(dist, base_row), _panel_ptr(ncomp, base_row), int(ld), int(n), int(row_begin), int(row_end),
                                       int(col_begin), int(dist_threshold), int(min_sites), _stream()))


def coo_from_dense(dist, ncomp, n, dist_threshold=2147483647, row_begin=0, row_end=None, col_begin=0, base_row=0):
    """-> rows, cols, d, nn (torch.int32 on device), row-major like the reference's output."""
    L = _lib.require_gpu()
    row_end = n if row_end is None else row_end
    nrows = max(0, row_end - row_begin)
    off = torch.zeros(nrows + 1, dtype=torch.int64, device=dist.device)
    ld = dist.stride(0)
    _lib.check(L.tracs_coo_count(_panel_ptr(dist, base_row), ld, n, row_begin, row_end, col_begin, int(dist_threshold), _ptr(off), _stream()))
    total = int(off[nrows].item())
    out = [torch.empty(total, dtype=torch.int32, device=dist.device) for _ in range(4)]
    if total:
        _lib.check(L.tracs_coo_fill(_panel_ptr(dist, base_row), _panel_ptr(ncomp, base_row), ld, n, row_begin, row_end, col_begin,
                                    int(dist_threshold), _ptr(off), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _stream()))
    return out


def knn_init(n_lists, k, device=None):
    """An empty k-nearest-neighbour state for samples [0, n_lists) (tracs_knn_init): a torch.uint8 device buffer."""
    L = _lib.require_gpu()
    nbytes = L.tracs_knn_state_bytes(int(n_lists), int(k))
    if nbytes == 0 and n_lists:
        raise ValueError("knn_init(): k must be in [1, 1024], got %d" % int(k))
    state = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device if device is not None else "cuda")
    _lib.check(L.tracs_knn_init(_ptr(state), int(n_lists), int(k), _stream()))
    return state


def knn_update(state, dist, ncomp, n, k, row_begin=0, row_end=None, col_begin=0, dist_threshold=2147483647, symmetric=True,
               base_row=0):
    """Merge the panel rows [row_begin, row_end) of dist / ncomp (as tracs_pairsnp_dense writes them; the panels hold rows
    base_row..) into the lists (tracs_knn_update).  symmetric: one-file mode, column c offers its cells to list c as well."""
    L = _lib.require_gpu()
    row_end = n if row_end is None else row_end
    ld = dist.stride(0)
    assert ncomp.stride(0) == ld
    _lib.check(L.tracs_knn_update(_panel_ptr(dist, base_row), _panel_ptr(ncomp, base_row), ld, n, row_begin, row_end, col_begin,
                                  int(dist_threshold), int(k), int(bool(symmetric)), _ptr(state), _stream()))


def knn_emit(state, k, list_begin, list_end):
    """Lists [list_begin, list_end) -> rows, cols, d, nn (torch.int32 on device), by list, each list by (d, j) (tracs_knn_emit)."""
    L = _lib.require_gpu()
    nl = max(0, int(list_end) - int(list_begin))
    off = torch.zeros(nl + 1, dtype=torch.int64, device=state.device)
    out = [torch.empty(max(nl * int(k), 1), dtype=torch.int32, device=state.device) for _ in range(4)]
    _lib.check(L.tracs_knn_emit(_ptr(state), int(list_begin), int(list_end), int(k), _ptr(off), _ptr(out[0]), _ptr(out[1]),
                                _ptr(out[2]), _ptr(out[3]), _stream()))
    total = int(off[nl].item())
    return [o[:total] for o in out]


def msf_init(n, device=None):
    """An empty minimum-spanning-forest state for the vertices [0, n) (tracs_msf_init): a torch.uint8 device buffer."""
    L = _lib.require_gpu()
    state = torch.empty(max(L.tracs_msf_state_bytes(int(n)), 1), dtype=torch.uint8, device=device if device is not None else "cuda")
    _lib.check(L.tracs_msf_init(_ptr(state), int(n), _stream()))
    return state


def _check_pair_batch(rows, cols, key, e_mask, d, nn, filt, p, e):
    """The tensor checks msf_update and anc_update share.  -> the batch's length, whether `key` (the weight / value) is float64"""
    m = int(rows.numel())
    assert cols.numel() == m and key.numel() == m
    for t in (rows, cols, key, e_mask, d, nn, filt, p, e):
        assert t is None or (t.is_contiguous() and t.numel() == m)
    for t in (rows, cols, d, nn, filt):
        assert t is None or t.element_size() == 4
    for t in (e_mask, p, e):
        assert t is None or t.dtype == torch.float64
    is_f64 = key.dtype == torch.float64
    assert is_f64 or (key.element_size() == 4 and not key.is_floating_point())
    return m, is_f64


def msf_update(state, n, rows, cols, weight, e_mask=None, e_max=-1.0, d=None, nn=None, filt=None, p=None, e=None):
    """F <- MSF(F u batch) (tracs_msf_update_coo): rows / cols int32 or uint32 device tensors, weight uint32-valued (int32 / uint32
    tensor, read as unsigned) or float64; e_mask (float64): only pairs with e_max >= e_mask are eligible.  d, nn, filt (32-bit) and
    p, e (float64) are the values kept with a pair.  -> the batch's eligible pairs."""
    L = _lib.require_gpu()
    m, is_f64 = _check_pair_batch(rows, cols, weight, e_mask, d, nn, filt, p, e)
    kind = 1 if is_f64 else 0
    taken = C.c_uint64(0)
    _lib.check(L.tracs_msf_update_coo(_ptr(state), int(n), m, _ptr(rows), _ptr(cols), _ptr(weight), kind, _ptr(e_mask), float(e_max),
                                      _ptr(d), _ptr(nn), _ptr(filt), _ptr(p), _ptr(e), C.byref(taken), _stream()))
    return taken.value


def msf_emit(state, n):
    """The forest in (i, j) order (tracs_msf_emit): rows < cols, d, nn, filt (torch.int32) and p, e (torch.float64) on the device."""
    L = _lib.require_gpu()
    cnt = C.c_size_t(0)
    _lib.check(L.tracs_msf_emit(_ptr(state), int(n), C.byref(cnt), *([C.c_void_p(0)] * 7), _stream()))
    k = cnt.value
    u = [torch.empty(max(k, 1), dtype=torch.int32, device=state.device) for _ in range(5)]
    f = [torch.empty(max(k, 1), dtype=torch.float64, device=state.device) for _ in range(2)]
    _lib.check(L.tracs_msf_emit(_ptr(state), int(n), C.byref(cnt), *[_ptr(t) for t in u + f], _stream()))
    return [t[:k] for t in u + f]


def anc_init(n, days, device=None):
    """A state without any offered pair for the vertices [0, n) (tracs_anc_init): a torch.uint8 device buffer.  days: torch.int32
    device tensor of n sampling days (days since 1970-01-01; copied into the state)."""
    L = _lib.require_gpu()
    assert days.dtype == torch.int32 and days.is_contiguous() and days.numel() == int(n)
    state = torch.empty(max(L.tracs_anc_state_bytes(int(n)), 1), dtype=torch.uint8, device=device if device is not None else days.device)
    _lib.check(L.tracs_anc_init(_ptr(state), int(n), _ptr(days), _stream()))
    return state


def anc_update(state, n, rows, cols, value, descending=False, e_mask=None, e_max=-1.0, d=None, nn=None, filt=None, p=None, e=None):
    """Offer a batch of pairs to every later-dated endpoint (tracs_anc_update_coo): rows / cols int32 or uint32 device tensors, value
    uint32-valued (int32 / uint32 tensor, read as unsigned, ascending) or float64 (ascending, or descending=True); e_mask (float64):
    only pairs with e_max >= e_mask are eligible.  d, nn, filt (32-bit) and p, e (float64) are the values kept with a pair.  -> the
    candidates offered (the batch's eligible pairs with unequal days)."""
    L = _lib.require_gpu()
    m, is_f64 = _check_pair_batch(rows, cols, value, e_mask, d, nn, filt, p, e)
    assert is_f64 or not descending
    kind = (2 if descending else 1) if is_f64 else 0
    taken = C.c_uint64(0)
    _lib.check(L.tracs_anc_update_coo(_ptr(state), int(n), m, _ptr(rows), _ptr(cols), _ptr(value), kind, _ptr(e_mask), float(e_max),
                                      _ptr(d), _ptr(nn), _ptr(filt), _ptr(p), _ptr(e), C.byref(taken), _stream()))
    return taken.value


def anc_emit(state, n):
    """The links in (i, j) order and the trees (tracs_anc_emit): rows < cols, d, nn, filt (torch.int32), p, e (torch.float64), then
    parent (-1 for a root), root and generation (torch.int32[n]), all on the device."""
    L = _lib.require_gpu()
    cnt = C.c_size_t(0)
    _lib.check(L.tracs_anc_emit(_ptr(state), int(n), C.byref(cnt), *([C.c_void_p(0)] * 10), _stream()))
    k = cnt.value
    u = [torch.empty(max(k, 1), dtype=torch.int32, device=state.device) for _ in range(5)]
    f = [torch.empty(max(k, 1), dtype=torch.float64, device=state.device) for _ in range(2)]
    t = [torch.empty(max(int(n), 1), dtype=torch.int32, device=state.device) for _ in range(3)]
    _lib.check(L.tracs_anc_emit(_ptr(state), int(n), C.byref(cnt), *[_ptr(x) for x in u + f + t], _stream()))
    return [x[:k] for x in u + f] + [x[:int(n)] for x in t]


TREE_METHODS = ("nj", "bionj")         # what --tree, DistanceHandle.tree(method=) and api.neighbor_joining(method=) take


def nj_init(n, device=None, method="nj"):
    """A neighbour-joining state with the zero matrix for the leaves [0, n) (tracs_nj_init): a torch.uint8 device buffer.  method
    "bionj": a state of tracs_bionj_state_bytes, which bionj_run needs (every other nj_* call serves both)."""
    if method not in TREE_METHODS:
        raise ValueError("nj_init(): method is 'nj' or 'bionj'")
    L = _lib.require_gpu()
    nbytes = (L.tracs_bionj_state_bytes if method == "bionj" else L.tracs_nj_state_bytes)(int(n))
    if nbytes == 0:
        raise ValueError("nj_init(): at most 2^24 leaves, got %d" % int(n))
    state = torch.empty(nbytes, dtype=torch.uint8, device=device if device is not None else "cuda")
    _lib.check(L.tracs_nj_init(_ptr(state), int(n), _stream()))
    return state


def nj_load_panel(state, n, dist, ncomp=None, row_begin=0, row_end=None, per_site=False, base_row=0):
    """The cells j > i of the panel rows [row_begin, row_end) of dist / ncomp (as pairsnp_dense wrote them; the panels hold rows
    base_row..) into the matrix, mirrored (tracs_nj_load_panel): D = d, or with per_site d / nn."""
    L = _lib.require_gpu()
    row_end = n if row_end is None else row_end
    ld = dist.stride(0)
    assert dist.element_size() == 4 and base_row <= row_begin and row_end - base_row <= dist.shape[0]
    assert ncomp is None or (ncomp.stride(0) == ld and ncomp.element_size() == 4)
    _lib.check(L.tracs_nj_load_panel(_ptr(state), int(n), _panel_ptr(dist, base_row), _panel_ptr(ncomp, base_row), int(ld), int(row_begin),
                                     int(row_end), int(bool(per_site)), _stream()))


def nj_load_f64(state, n, matrix):
    """The cells j > i of a torch.float64 device matrix [n, ld >= n] into the matrix, mirrored (tracs_nj_load_f64)."""
    L = _lib.require_gpu()
    assert matrix.dtype == torch.float64 and matrix.dim() == 2 and matrix.stride(1) == 1 and matrix.shape[0] >= n and matrix.shape[1] >= n
    _lib.check(L.tracs_nj_load_f64(_ptr(state), int(n), _ptr(matrix), int(matrix.stride(0)), _stream()))


def nj_run(state, n):
    """The row sums and the n - 3 joins, enqueued on the current stream (tracs_nj_run)."""
    _lib.check(_lib.require_gpu().tracs_nj_run(_ptr(state), int(n), _stream()))


def bionj_run(state, n):
    """nj_run with the BIONJ reduction (tracs_bionj_run): state from nj_init(n, method="bionj")."""
    if state.numel() < _lib.require_gpu().tracs_bionj_state_bytes(int(n)):
        raise ValueError("bionj_run(): the state is smaller than a BIONJ state for %d leaves" % int(n))
    _lib.check(_lib.require_gpu().tracs_bionj_run(_ptr(state), int(n), _stream()))


def nj_emit(state, n):
    """The join records and the last three nodes (tracs_nj_emit), on the host: (a, b (uint32), d_ab, r_a, r_b (float64)), last_ids
    (uint32[3]), last_d (float64[3]).  A per-site cell with nn = 0: ValueError carrying .pair = (i, j)."""
    L = _lib.require_gpu()
    m = max(int(n) - 3, 0)
    a, b = np.zeros(max(m, 1), np.uint32), np.zeros(max(m, 1), np.uint32)
    f = [np.zeros(max(m, 1), np.float64) for _ in range(3)]
    last_ids, last_d, zero = np.zeros(3, np.uint32), np.zeros(3, np.float64), np.zeros(2, np.uint32)
    cnt = C.c_size_t(0)
    rc = L.tracs_nj_emit(_ptr(state), int(n), C.byref(cnt), *[C.c_void_p(x.ctypes.data) for x in [a, b] + f + [last_ids, last_d, zero]],
                         _stream())
    if rc and zero[0] != 0xFFFFFFFF:
        err = ValueError("nj_emit(): samples %d and %d were compared over 0 sites: no per-site distance" % (zero[0], zero[1]))
        err.pair = (int(zero[0]), int(zero[1]))
        raise err
    _lib.check(rc)
    return (a[:m], b[:m], f[0][:m], f[1][:m], f[2][:m]), last_ids, last_d


def nj_edges(n, records, last_ids, last_d):
    """Branch lengths from nj_emit's output (tracs_nj_edges; host only) -> parent, child (uint32), length (float64): the tree's
    2n - 3 edges in creation order (join t makes node n + t, the top node is 2n - 3)."""
    L = _lib.load()
    cap = max(2 * int(n), 1)
    parent, child, length = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.float64)
    arrs = [np.ascontiguousarray(x, dt) for x, dt in zip(records, (np.uint32, np.uint32, np.float64, np.float64, np.float64))]
    arrs += [np.ascontiguousarray(last_ids, np.uint32), np.ascontiguousarray(last_d, np.float64)]
    cnt = C.c_size_t(0)
    _lib.check(L.tracs_nj_edges(int(n), *[C.c_void_p(x.ctypes.data) for x in arrs + [parent, child, length]], C.byref(cnt)))
    return parent[:cnt.value], child[:cnt.value], length[:cnt.value]


def hist_init(n_bins, device=None):
    """An all-zero histogram state for the values [0, n_bins) (tracs_hist_init): a torch.uint8 device buffer."""
    L = _lib.require_gpu()
    nbytes = L.tracs_hist_state_bytes(int(n_bins))
    if nbytes == 0:
        raise ValueError("hist_init(): n_bins must be in [1, 2^31], got %d" % int(n_bins))
    state = torch.empty(nbytes, dtype=torch.uint8, device=device if device is not None else "cuda")
    _lib.check(L.tracs_hist_init(_ptr(state), int(n_bins), _stream()))
    return state


def hist_update(state, n_bins, dist, n, row_begin=0, row_end=None, col_begin=0, dist_threshold=2147483647, group=None, base_row=0):
    """Count the cells of the panel rows [row_begin, row_end) of dist (as tracs_pairsnp_dense writes them; the panel holds rows
    base_row..) that are, read as unsigned, <= dist_threshold (tracs_hist_update).  group: torch.int32 device labels of the n
    samples (< 0: ungrouped) or None (every pair ungrouped)."""
    L = _lib.require_gpu()
    row_end = n if row_end is None else row_end
    assert dist.element_size() == 4 and dist.stride(1) == 1
    assert group is None or (group.dtype == torch.int32 and group.is_contiguous() and group.numel() == n)
    _lib.check(L.tracs_hist_update(_panel_ptr(dist, base_row), dist.stride(0), int(n), int(row_begin), int(row_end), int(col_begin),
                                   int(dist_threshold), _ptr(group), _ptr(state), int(n_bins), _stream()))


def hist_update_coo(state, n_bins, rows, cols, val, group=None):
    """Count the listed pairs (rows, cols) with their values val: 32-bit device vectors of equal length (tracs_hist_update_coo)."""
    L = _lib.require_gpu()
    m = int(val.numel())
    for t in (rows, cols, val):
        assert t.is_contiguous() and t.numel() == m and t.element_size() == 4 and not t.is_floating_point()
    assert group is None or (group.dtype == torch.int32 and group.is_contiguous())
    _lib.check(L.tracs_hist_update_coo(_ptr(rows), _ptr(cols), _ptr(val), m, _ptr(group), _ptr(state), int(n_bins), _stream()))


def hist_emit(state, n_bins):
    """The non-empty bins, ascending (tracs_hist_emit): value (torch.int32, bit pattern uint32), within, between, ungrouped
    (torch.int64, bit pattern uint64) on the device.  RuntimeError when a value >= n_bins was offered."""
    L = _lib.require_gpu()
    cnt = C.c_size_t(0)
    _lib.check(L.tracs_hist_emit(_ptr(state), int(n_bins), C.byref(cnt), *([C.c_void_p(0)] * 4), _stream()))
    k = cnt.value
    value = torch.empty(max(k, 1), dtype=torch.int32, device=state.device)
    counts = [torch.empty(max(k, 1), dtype=torch.int64, device=state.device) for _ in range(3)]
    if k:
        _lib.check(L.tracs_hist_emit(_ptr(state), int(n_bins), C.byref(cnt), _ptr(value), *[_ptr(t) for t in counts], _stream()))
    return [value[:k]] + [t[:k] for t in counts]


def hist_routes(state):
    """The cells the updates of `state` counted by each route of csrc/histogram.hip, and its LDS slots per class (tests only)."""
    out = (C.c_double * 4)()
    if _lib.require_gpu().tracs_debug_hist_routes(_ptr(state), out) != 4:
        return None
    return {"combined": int(out[0]), "lds": int(out[1]), "global": int(out[2]), "window": int(out[3])}


def edges_from_dense_f64(val, dist, n, threshold, dist_threshold=2147483647, row_begin=0, row_end=None, col_begin=0, base_row=0,
                         with_values=False):
    """Cells (i, j > i) with dist <= dist_threshold and val <= threshold, row-major -> rows, cols (torch.int32)[, values f64]:
    the edges `tracs cluster -D expectedK|direct -c threshold` keeps (tracs/cluster.py:110-112), straight from device panels."""
    L = _lib.require_gpu()
    row_end = n if row_end is None else row_end
    nrows = max(0, row_end - row_begin)
    off = torch.zeros(nrows + 1, dtype=torch.int64, device=val.device)
    ld = val.stride(0)
    assert dist.stride(0) == ld
    _lib.check(L.tracs_edges_count_f64(_panel_ptr(val, base_row), _panel_ptr(dist, base_row), ld, n, row_begin, row_end, col_begin,
                                       int(dist_threshold), float(threshold), _ptr(off), _stream()))
    total = int(off[nrows].item())
    rows = torch.empty(total, dtype=torch.int32, device=val.device)
    cols = torch.empty(total, dtype=torch.int32, device=val.device)
    vals = torch.empty(total, dtype=torch.float64, device=val.device) if with_values else None
    if total:
        _lib.check(L.tracs_edges_fill_f64(_panel_ptr(val, base_row), _panel_ptr(dist, base_row), ld, n, row_begin, row_end, col_begin,
                                          int(dist_threshold), float(threshold), _ptr(off), _ptr(rows), _ptr(cols), _ptr(vals), _stream()))
    return (rows, cols, vals) if with_values else (rows, cols)


def filter_recomb_device(aln, rows, cols, d):
    """rows/cols/d: torch.int32 device vectors of emitted pairs -> filtered distances (torch.int32)."""
    L = _lib.require_gpu()
    n = rows.numel()
    off = torch.zeros(n + 1, dtype=torch.int64, device=rows.device)
    off[1:] = torch.cumsum(d.to(torch.int64), 0)
    total = int(off[n].item()) if n else 0
    pos = torch.empty(max(total, 1), dtype=torch.int32, device=rows.device)
    found = torch.empty(max(n, 1), dtype=torch.int32, device=rows.device)
    filt = torch.empty(max(n, 1), dtype=torch.int32, device=rows.device)
    _lib.check(L.tracs_filter_recomb_device(aln._h, _ptr(rows), _ptr(cols), n, _ptr(off), _ptr(pos), _ptr(found), _ptr(filt),
                                            _stream()))
    return filt[:n], found[:n], pos[:total], off


def filter_recomb_pairs(aln, rows, cols, d):
    """Filtered distances (src/pairsnp.hpp:251-318) of the emitted pairs (rows, cols) with SNP distances d: torch.int32 device
    vectors in, torch.int32 out.  The pairs' SNP sites come from the samples' departure lists (csrc/filter_lists.hip), built on the
    alignment's first filter call after a pack."""
    L = _lib.require_gpu()
    n = rows.numel()
    filt = torch.empty(max(n, 1), dtype=torch.int32, device=rows.device)
    if n:
        _lib.check(L.tracs_filter_recomb_pairs(aln._h, _ptr(rows), _ptr(cols), _ptr(d), n, _ptr(filt), _stream()))
    return filt[:n]


def pair_sites(aln, rows, cols, filter=False):
    """The SNP sites of the listed pairs (rows, cols: 32-bit device vectors of sample indices, either order, repeats allowed) ->
    (offsets torch.int64 [m + 1], site, info torch.int32) on the device: pair t's entries are [offsets[t], offsets[t + 1]), ascending
    by site -- the sites at which the two samples' allele sets are disjoint, so their number is the pair's SNP distance.  info: bits
    0-3 the rows[t] sample's allele mask, bits 4-7 the cols[t] sample's (A = 1, C = 2, G = 4, T = 8); with filter, bit 8 is set on
    the SNPs the recombination filter drops.  tracs_pair_sites_count / _fill (csrc/pair_sites.hip)."""
    L = _lib.require_gpu()
    m = int(rows.numel())
    assert cols.numel() == m
    for t in (rows, cols):
        assert t.is_cuda and t.is_contiguous() and t.element_size() == 4 and not t.is_floating_point()
    d = torch.empty(max(m, 1), dtype=torch.int32, device=rows.device)
    off = torch.empty(m + 1, dtype=torch.int64, device=rows.device)
    total = C.c_uint64(0)
    _lib.check(L.tracs_pair_sites_count(aln._h, _ptr(rows), _ptr(cols), m, _ptr(d), _ptr(off), C.byref(total), _stream()))
    k = int(total.value)
    site = torch.empty(max(k, 1), dtype=torch.int32, device=rows.device)
    info = torch.empty(max(k, 1), dtype=torch.int32, device=rows.device)
    if k:
        _lib.check(L.tracs_pair_sites_fill(aln._h, _ptr(rows), _ptr(cols), m, _ptr(off), 0, _ptr(site), _ptr(info), k, int(bool(filter)),
                                           _stream()))
    return off, site[:k], info[:k]


def _tree_arrays(parent, child):
    parent, child = np.ascontiguousarray(parent, np.uint32), np.ascontiguousarray(child, np.uint32)
    if parent.ndim != 1 or parent.shape != child.shape:
        raise ValueError("parent and child must be two arrays of one length")
    return parent, child


def fitch_count(aln, parent, child):
    """Every site of the alignment placed on a tree over its samples by Fitch's two passes (tracs_fitch_count).  parent,
    child: the edges as nj_edges returns them (host arrays).  -> (edge_changes torch.int32 [2n - 3], site_changes torch.int32 [L],
    site_minimum torch.uint8 [L], offsets torch.int64 [L + 1], total) on the device: the changes on every edge and at every site, the
    fewest changes any tree needs at the site, and the exclusive scan of site_changes (total = offsets[L], the tree's parsimony
    length)."""
    L = _lib.require_gpu()
    parent, child = _tree_arrays(parent, child)
    ne, sites = len(parent), int(aln.L)
    dev = "cuda"
    edge = torch.zeros(max(ne, 1), dtype=torch.int32, device=dev)
    site = torch.zeros(max(sites, 1), dtype=torch.int32, device=dev)
    minimum = torch.zeros(max(sites, 1), dtype=torch.uint8, device=dev)
    off = torch.zeros(sites + 1, dtype=torch.int64, device=dev)
    total = C.c_uint64(0)
    _lib.check(L.tracs_fitch_count(aln._h, parent.ctypes.data, child.ctypes.data, ne, _ptr(edge), _ptr(site), _ptr(minimum), _ptr(off),
                                   C.byref(total), _stream()))
    return edge[:ne], site[:sites], minimum[:sites], off, int(total.value)


def fitch_fill(aln, parent, child, off, site_begin=0, site_end=None, entry_base=None, room=None, out=None):
    """The changes of the sites [site_begin, site_end) (tracs_fitch_fill), after fitch_count gave `off`: -> (site, edge, info) torch.int32
    on the device, the entries of site s at [off[s] - entry_base, off[s + 1] - entry_base) in the order of the top-down walk: the site,
    the index into the edge list, and the parent's state in bits 0-3 / the child's in bits 4-7 of info (one-hot, A = 1 ... T = 8).
    entry_base: off[site_begin] by default; room: the entries the buffers hold (by default what the range needs); out: three buffers
    to fill instead of new ones (nothing is written beyond room)."""
    L = _lib.require_gpu()
    parent, child = _tree_arrays(parent, child)
    sites = int(aln.L)
    site_end = sites if site_end is None else int(site_end)
    if entry_base is None:
        entry_base = int(off[site_begin].item()) if sites else 0
    need = (int(off[site_end].item()) - int(entry_base)) if sites else 0
    room = max(need, 0) if room is None else int(room)
    if out is None:
        out = tuple(torch.zeros(max(room, 1), dtype=torch.int32, device=off.device) for _ in range(3))
    for t in out:
        assert t.is_cuda and t.is_contiguous() and t.element_size() == 4 and t.numel() >= room
    _lib.check(L.tracs_fitch_fill(aln._h, parent.ctypes.data, child.ctypes.data, len(parent), int(site_begin), site_end, _ptr(off),
                                  int(entry_base), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), room, _stream()))
    torch.cuda.current_stream().synchronize()              # (the edges are host arrays of this call)
    k = max(min(need, room), 0)
    return out[0][:k], out[1][:k], out[2][:k]


def fitch_edge_sites(aln, parent, child, edge_changes, room=None, out=None):
    """The changes regrouped by edge (tracs_fitch_edge_sites), after fitch_count gave edge_changes: -> (edge_off torch.int64
    [n_edges + 1], edge_site torch.int32) on the device, the sites with a change on edge e at [edge_off[e], edge_off[e + 1]), ascending.
    room: the entries edge_site holds (by default the total); out: a buffer to fill instead of a new one (nothing is written beyond
    room)."""
    L = _lib.require_gpu()
    parent, child = _tree_arrays(parent, child)
    ne = len(parent)
    assert edge_changes.is_cuda and edge_changes.is_contiguous() and edge_changes.element_size() == 4 and edge_changes.numel() >= ne
    total = int(edge_changes[:ne].to(torch.int64).sum().item()) if ne else 0
    room = total if room is None else int(room)
    edge_off = torch.zeros(ne + 1, dtype=torch.int64, device=edge_changes.device)
    if out is None:
        out = torch.zeros(max(room, 1), dtype=torch.int32, device=edge_changes.device)
    assert out.is_cuda and out.is_contiguous() and out.element_size() == 4 and out.numel() >= room
    _lib.check(L.tracs_fitch_edge_sites(aln._h, parent.ctypes.data, child.ctypes.data, ne, _ptr(edge_changes), _ptr(edge_off), _ptr(out), room,
                                        _stream()))
    torch.cuda.current_stream().synchronize()              # (the edges are host arrays of this call)
    return edge_off, out[:min(total, room)]


def filter_recomb_lists(aln, off, pos, with_dropped=True):
    """The recombination filter (src/pairsnp.hpp:251-318) on sorted position lists (tracs_filter_recomb_lists): list t is
    pos[off[t] : off[t + 1]] (off torch.int64 [m + 1] from 0, pos 32-bit, both on the device; every list ascending and below aln.L)
    -> (filt torch.int32 [m], the entries kept per list; dropped torch.uint8 [len(pos)], 1 on the entries dropped, or None)."""
    L = _lib.require_gpu()
    m = int(off.numel()) - 1
    assert m >= 0 and off.is_cuda and off.is_contiguous() and off.dtype == torch.int64
    assert pos.is_cuda and pos.is_contiguous() and pos.element_size() == 4 and not pos.is_floating_point()
    k = int(pos.numel())
    filt = torch.zeros(max(m, 1), dtype=torch.int32, device=off.device)
    dropped = torch.zeros(max(k, 1), dtype=torch.uint8, device=off.device) if with_dropped else None
    if m:
        _lib.check(L.tracs_filter_recomb_lists(aln._h, _ptr(off), _ptr(pos), m, k, _ptr(filt), _ptr(dropped), _stream()))
    return filt[:m], (dropped[:k] if with_dropped else None)


def fitch_mark_dropped(site, edge, info, edge_off, edge_site, dropped):
    """Bit 8 of info on the entries of fitch_fill that the branch filter drops (tracs_fitch_mark_dropped): in place, -> info."""
    L = _lib.require_gpu()
    k = int(info.numel())
    assert site.numel() == k and edge.numel() == k
    _lib.check(L.tracs_fitch_mark_dropped(_ptr(site), _ptr(edge), _ptr(info), k, int(edge_off.numel()) - 1, _ptr(edge_off), _ptr(edge_site),
                                          _ptr(dropped), _stream()))
    return info


def clone_alignment(aln):
    """-> a new Alignment with the n, L and planes of `aln`, byte for byte (a device-to-device copy; tracs_alignment_clone); `aln` is
    left as it was.  A copy that does not fit in the device's memory is refused."""
    h = C.c_void_p()
    _lib.check(aln._L.tracs_alignment_clone(aln._h, C.byref(h), _stream()))
    new = Alignment.__new__(Alignment)
    new._L, new._h = aln._L, h
    new.n, new.L = aln.n, aln.L
    for attr in ("names", "n_first"):
        if hasattr(aln, attr):
            setattr(new, attr, getattr(aln, attr))
    return new


def restore_alignment(dst, src):
    """dst's planes <- src's (two handles of one shape; tracs_alignment_restore): a clone put back to its source after mask_subtrees"""
    _lib.check(dst._L.tracs_alignment_restore(dst._h, src._h, _stream()))


def mask_subtrees(aln, parent, child, edge_off, edge_site, dropped):
    """The branch filter's verdicts into the alignment, in place (tracs_alignment_mask_subtrees): for every entry k with
    dropped[k] != 0 of edge e (edge_off torch.int64 [n_edges + 1], edge_site 32-bit, dropped torch.uint8, on the device: what
    fitch_edge_sites and filter_recomb_lists return) the cell (i, edge_site[k]) becomes N for every sample i below e, the side away
    from the tree's top node.  parent, child: the edges as nj_edges returns them (host arrays).  -> the cells that were not N and now
    are.  What the handle caches per pack is rebuilt by its next call."""
    L = _lib.require_gpu()
    parent, child = _tree_arrays(parent, child)
    k = int(edge_site.numel())
    assert edge_off.is_cuda and edge_off.is_contiguous() and edge_off.dtype == torch.int64
    assert k == 0 or (edge_site.is_cuda and edge_site.is_contiguous() and edge_site.element_size() == 4 and not edge_site.is_floating_point())
    assert int(dropped.numel()) >= k and (k == 0 or (dropped.is_cuda and dropped.is_contiguous() and dropped.dtype == torch.uint8))
    cells = C.c_uint64(0)
    _lib.check(L.tracs_alignment_mask_subtrees(aln._h, parent.ctypes.data, child.ctypes.data, len(parent), _ptr(edge_off), _ptr(edge_site),
                                               _ptr(dropped), k, C.byref(cells), _stream()))
    return int(cells.value)


def filter_index_info(aln):
    """Diagnostics of the alignment's filter index (None before the first filter call)."""
    import ctypes as C
    L = _lib.require_gpu()
    out = (C.c_double * 10)()
    if not L.tracs_debug_filter_index(aln._h, out):
        return None
    keys = ("ref", "count", "offsets", "fill", "nt", "ns")
    return {"lists": bool(out[0]), "entries": int(out[1]), "longest_list": int(out[2]), "alloc_ms": out[3],
            "build_ms": {k: out[4 + i] for i, k in enumerate(keys)}}


def trans_dist_device(snpdiff, datediff, lamb, beta, threshold_Ek, exp_p0=False):
    L = _lib.require_gpu()
    n = snpdiff.numel()
    p0 = torch.empty(n, dtype=torch.float64, device=snpdiff.device)
    eK = torch.empty(n, dtype=torch.float64, device=snpdiff.device)
    _lib.check(L.tracs_trans_dist_device(_ptr(snpdiff), _ptr(datediff), n, float(lamb), float(beta), float(threshold_Ek),
                                         int(exp_p0), _ptr(p0), _ptr(eK), _stream()))
    return p0, eK


def trans_routes():
    """How the last transcluster call evaluated its distinct keys (csrc/transcluster.hip tracs_debug_trans_routes; tests only)."""
    out = (C.c_double * 8)()
    if _lib.require_gpu().tracs_debug_trans_routes(out) != 8:
        return None
    v = [int(x) for x in out]
    return {"keys": v[0], "serial": v[1], "ratio": v[2], "ratio_zero": v[3], "wave": v[4], "tables": bool(v[5]),
            "linear": bool(v[6]), "route": "grid" if v[7] else "hash"}


def trans_dist_dense(dist, n, days, lamb, beta, threshold_Ek, p0, eK, exp_p0=True, dist_threshold=2147483647,
                     row_begin=0, row_end=None, col_begin=0, base_row=0):
    L = _lib.require_gpu()
    row_end = n if row_end is None else row_end
    ld = dist.stride(0)
    assert p0.stride(0) == ld and eK.stride(0) == ld
    _lib.check(L.tracs_trans_dist_dense(_panel_ptr(dist, base_row), ld, n, row_begin, row_end, col_begin, int(dist_threshold), _ptr(days),
                                        float(lamb), float(beta), float(threshold_Ek), int(exp_p0), _panel_ptr(p0, base_row),
                                        _panel_ptr(eK, base_row), _stream()))


def trans_dist_dense_ranges(dist, n, days, lamb, beta, threshold_Ek, p0, eK, ranges, exp_p0=True,
                            dist_threshold=2147483647, col_begin=0):
    """One pass (one key table) over one or two row panels: ranges = [(b0, e0)] or [(b0, e0), (b1, e1)]."""
    L = _lib.require_gpu()
    ld = dist.stride(0)
    assert p0.stride(0) == ld and eK.stride(0) == ld and 1 <= len(ranges) <= 2
    flat = [int(x) for r in ranges for x in r]
    arr = (C.c_size_t * len(flat))(*flat)
    _lib.check(L.tracs_trans_dist_dense2(_ptr(dist), ld, n, arr, len(ranges), col_begin, int(dist_threshold), _ptr(days),
                                         float(lamb), float(beta), float(threshold_Ek), int(exp_p0), _ptr(p0), _ptr(eK),
                                         _stream()))


def trans_dist_dense_partitioned(dist, n, days, lamb, beta, threshold_Ek, p0, eK, part, parts, all_reduce, exp_p0=True,
                                 dist_threshold=2147483647, n_max=None, d_max=None):
    """trans_dist_dense over the WHOLE matrix on every rank, with the key evaluations split over the ranks: this rank evaluates
    the keys of hash class `part` of `parts` into a dense key table, `all_reduce(tensor)` sums the tables over the ranks
    (torch.distributed: RCCL), and p0 / eK of every cell are read from the completed table."""
    L = _lib.require_gpu()
    ld = dist.stride(0)
    assert p0.stride(0) == ld and eK.stride(0) == ld
    if n_max is None:
        valid = torch.triu(dist[:n, :n], diagonal=1)
        n_max = int(torch.where(valid <= dist_threshold, valid, torch.zeros_like(valid)).max().item())
    if d_max is None:
        d_max = int((days.max() - days.min()).item())
    table = torch.zeros((2, n_max + 1, d_max + 1), dtype=torch.float64, device=dist.device)
    flag = torch.zeros(1, dtype=torch.int32, device=dist.device)
    _lib.check(L.tracs_trans_table_dense(_ptr(dist), ld, n, 0, n, 0, int(dist_threshold), _ptr(days), float(lamb), float(beta),
                                         float(threshold_Ek), int(part), int(parts), n_max, d_max, _ptr(table[0]), _ptr(table[1]),
                                         _ptr(flag), _stream()))
    if parts > 1:
        all_reduce(table)
    _lib.check(L.tracs_trans_table_gather(_ptr(dist), ld, n, 0, n, 0, int(dist_threshold), _ptr(days), n_max, d_max, _ptr(table[0]),
                                          _ptr(table[1]), int(exp_p0), _ptr(p0), _ptr(eK), _ptr(flag), _stream()))
    if int(flag.item()):
        raise _lib.TracsError("trans_dist key table too small (n_max / d_max)")


# ---- the distinct keys split over ranks that each hold rows of the matrix (partition.KeySplit; csrc/transcluster.hip) ---------------
def trans_keys_words():
    return int(_lib.require_gpu().tracs_trans_keys_words())


def _ranges_arg(ranges):
    flat = [int(x) for r in ranges for x in r]
    return (C.c_size_t * max(1, len(flat)))(*flat), len(ranges)


def trans_keys_mark(dist, n, days, ranges, keys, dist_threshold=2147483647, col_begin=0):
    """keys (torch.int32 [trans_keys_words()], overwritten) <- the (SNP distance, day gap) keys of the cells of the row ranges"""
    L = _lib.require_gpu()
    assert len(ranges) <= 2 and keys.is_contiguous() and keys.numel() == trans_keys_words()
    arr, k = _ranges_arg(ranges)
    _lib.check(L.tracs_trans_keys_mark(_ptr(dist), dist.stride(0), n, arr, k, col_begin, int(dist_threshold), _ptr(days), _ptr(keys), _stream()))


def trans_keys_merge(keys, gathered, parts):
    L = _lib.require_gpu()
    assert gathered.is_contiguous() and gathered.numel() == parts * keys.numel()
    _lib.check(L.tracs_trans_keys_merge(_ptr(keys), _ptr(gathered), int(parts), _stream()))


def trans_keys_info(keys):
    """-> (distinct keys, largest distance, span of the days, fits the grid) of a (merged) key bitmap; synchronises"""
    L = _lib.require_gpu()
    info = (C.c_uint64 * 4)()
    _lib.check(L.tracs_trans_keys_info(_ptr(keys), info, _stream()))
    return tuple(int(x) for x in info)


def trans_keys_evaluate(keys, info, part, parts, lamb, beta, threshold_Ek, vals):
    """vals (torch.float64 [per, 2]) <- (log p0, E(K)) of the keys with ordinal = part mod parts, at slot ordinal // parts"""
    L = _lib.require_gpu()
    assert vals.is_contiguous() and vals.dtype == torch.float64
    arr = (C.c_uint64 * 4)(*info)
    _lib.check(L.tracs_trans_keys_evaluate(_ptr(keys), arr, int(part), int(parts), float(lamb), float(beta), float(threshold_Ek),
                                           _ptr(vals), vals.numel() // 2, _stream()))


def trans_keys_gather(dist, n, days, ranges, keys, info, vals_all, parts, p0, eK, exp_p0=True, dist_threshold=2147483647, col_begin=0):
    L = _lib.require_gpu()
    ld = dist.stride(0)
    assert p0.stride(0) == ld and eK.stride(0) == ld and len(ranges) <= 2 and vals_all.is_contiguous()
    arr, k = _ranges_arg(ranges)
    inf = (C.c_uint64 * 4)(*info)
    _lib.check(L.tracs_trans_keys_gather(_ptr(dist), ld, n, arr, k, col_begin, int(dist_threshold), _ptr(days), _ptr(keys), inf,
                                         _ptr(vals_all), int(parts), vals_all.numel() // (2 * parts), int(exp_p0), _ptr(p0), _ptr(eK), _stream()))


def calculate_posteriors_device(counts, alphas, keep, threshold):
    L = _lib.require_gpu()
    a = np.ascontiguousarray(alphas, dtype=np.float64)
    out = torch.empty_like(counts)
    _lib.check(L.tracs_calculate_posteriors_device(_ptr(counts), counts.shape[0], counts.shape[1],
                                                   a.ctypes.data_as(C.POINTER(C.c_double)), int(bool(keep)),
                                                   float(threshold), _ptr(out), _stream()))
    return out


def posterior_codes_device(counts_u16, alphas, keep, threshold, min_cov=0, cov_band=None, out=None):
    """counts_u16: torch.int16/uint16 [L,4] (or int32 [L,4] for depths above 65535) -> torch.uint8 [(L+1)//2] packed allele
    masks (low nibble = even site).  min_cov / cov_band=(lo, hi): the align stage's coverage rules (sites below min_cov or
    inside the band become N).  out: a contiguous uint8 view of at least (L+1)//2 bytes to write into (e.g. the sample's row
    of a batch buffer for Alignment.pack_codes)."""
    L = _lib.require_gpu()
    a = np.ascontiguousarray(alphas, dtype=np.float64)
    n = counts_u16.shape[0]
    if out is None:
        out = torch.empty((n + 1) // 2, dtype=torch.uint8, device=counts_u16.device)
    else:
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= (n + 1) // 2 and out.device == counts_u16.device
    lo, hi = cov_band if cov_band is not None else (1.0, 0.0)
    assert counts_u16.is_contiguous() and counts_u16.element_size() in (2, 4)
    fn = L.tracs_posterior_codes_cov_device32 if counts_u16.element_size() == 4 else L.tracs_posterior_codes_cov_device
    _lib.check(fn(_ptr(counts_u16), n, a.ctypes.data_as(C.POINTER(C.c_double)), int(bool(keep)), float(threshold), int(min_cov),
                  float(lo), float(hi), _ptr(out), _stream()))
    return out


def codes_to_iupac_device(codes, L):
    """packed 4-bit masks -> torch.uint8 [L] IUPAC letters ('X' for an empty mask), tracs/align.py:285-323."""
    lib = _lib.require_gpu()
    out = torch.empty(L, dtype=torch.uint8, device=codes.device)
    _lib.check(lib.tracs_codes_to_iupac_device(_ptr(codes), L, _ptr(out), _stream()))
    return out


def connected_components_device(I, J, n_nodes):
    L = _lib.require_gpu()
    labels = torch.empty(n_nodes, dtype=torch.int32, device=I.device)
    nc = C.c_int32(0)
    _lib.check(L.tracs_connected_components_device(_ptr(I), _ptr(J), I.numel(), n_nodes, _ptr(labels), C.byref(nc), _stream()))
    return int(nc.value), labels


def tri_pack(mat, n, row_begin, row_end, col_begin, slots, width, base, negate, packed_ptr, stats, base_row=0):
    """csrc/exchange.hip: the cells (i, j >= max(col_begin, i + 1)) of rows [row_begin, row_end) of the uint32 panel `mat` (rows
    base_row..) -> `width` bytes per cell at element slots[i - row_begin] of the buffer at packed_ptr (None: only the statistics);
    stats: int32[2] (largest value, values beyond 16 bits)."""
    L = _lib.require_gpu()
    assert slots.dtype == torch.int64 and slots.is_contiguous() and slots.numel() == row_end - row_begin
    _lib.check(L.tracs_tri_pack(_panel_ptr(mat, base_row), int(mat.stride(0)), int(n), int(row_begin), int(row_end), int(col_begin), _ptr(slots),
                                int(width), int(base) & 0xFFFFFFFF, int(negate), C.c_void_p(packed_ptr or 0), _ptr(stats), _stream()))


def tri_sum(mat, n, row_begin, row_end, col_begin, slots, width, recv_ptr, block_elems, n_blocks, skip_block, add, negate, base_row=0):
    """csrc/exchange.hip: mat[i][j] += add +/- the sum over the blocks b != skip_block of recv[b * block_elems + slots[i - row_begin] + j - first
    column] for the rows whose slot is not -1."""
    L = _lib.require_gpu()
    assert slots.dtype == torch.int64 and slots.is_contiguous() and slots.numel() == row_end - row_begin
    _lib.check(L.tracs_tri_sum(_panel_ptr(mat, base_row), int(mat.stride(0)), int(n), int(row_begin), int(row_end), int(col_begin), _ptr(slots),
                               int(width), C.c_void_p(recv_ptr), int(block_elems), int(n_blocks), int(skip_block), int(add) & 0xFFFFFFFF,
                               int(negate), _stream()))
