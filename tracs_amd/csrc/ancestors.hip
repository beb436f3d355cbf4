// ancestors.hip -- each sample's most likely earlier source among the eligible pairs (tracs_anc_*, include/tracs_hip.h).
//
// For a sample s sampled on day t_s, a sample a is a candidate when {a, s} is an offered, eligible pair and t_a < t_s (strictly: equal
// days never link, so the links cannot form a cycle).  The chosen source is the smallest candidate under (value key, t_s - t_a, a): a
// strict total order, so the result does not depend on how the pairs are split into updates.  The value key is order-preserving in 64
// bits: a uint32 value as is; an f64 value through f64_key_up, or f64_key_down for the descending kind (pair_select.h).  (value, gap, a) does not fit in 64 bits, so the minimum is taken in two steps:
//   pass 1   per candidate pair: its later endpoint takes the value key (atomicMin)
//   settle   per vertex: a value key lowered by this update discards the tie key kept from earlier updates; one that stayed keeps it
//   pass 2   per candidate pair that ties its later endpoint's value key: the endpoint takes gap << 32 | a (atomicMin)
//   pass 3   the pair that won a vertex records its index in the batch (unique: every pair is offered once)
//   gather   per vertex with a winner in this batch: the parent and the pair's values are copied from the batch
// Every pair has one atomic target (its later endpoint).  Atomics are reduced across the wave first (wave_min_into, pair_select.h): a
// segmented minimum over runs of one target leaves one atomic per run, and only when a plain read shows it can lower the target.
// Emit sorts the links by i << 32 | j (rocprim radix sort) and finds every vertex's root and generation by pointer doubling in
// ceil(log2 n) rounds -- a fixed bound, whatever the parent array holds.
#include "common.h"
#include "pair_select.h"

using namespace tracs;

namespace {

struct Hdr {
    unsigned long long n;           // vertices the state was initialised for
    unsigned long long taken;       // candidates offered by the running update
    unsigned long long links;       // vertices with a parent (counted by emit)
};

// State (capacity cap = max(n, 1)): header, days, per-vertex best keys, the winning pair's identity and values, then scratch for emit
// (sort keys and indices, two hop / generation buffers each)
struct State {
    Hdr *hdr;
    int *days;
    unsigned long long *bv, *bt, *cv, *keys;
    unsigned *win, *pa, *idx, *hop, *gen;
    PairColumns val;
    size_t cap;
    State(void *base, size_t n, size_t *bytes = nullptr)
    {
        cap = std::max<size_t>(n, 1);
        Arena a(base, bytes);
        hdr = reinterpret_cast<Hdr *>(a.take<char>(64));
        days = a.take<int>(cap);
        bv = a.take<unsigned long long>(cap); bt = a.take<unsigned long long>(cap); cv = a.take<unsigned long long>(cap);
        win = a.take<unsigned>(cap); pa = a.take<unsigned>(cap);
        val.d = a.take<unsigned>(cap); val.nn = a.take<unsigned>(cap); val.f = a.take<unsigned>(cap);
        val.p = a.take<double>(cap); val.e = a.take<double>(cap);
        keys = a.take<unsigned long long>(2 * cap); idx = a.take<unsigned>(2 * cap); hop = a.take<unsigned>(2 * cap); gen = a.take<unsigned>(2 * cap);
    }
};

// Pair t of the batch as a candidate: -> its later-dated endpoint (NO_VERTEX: not a candidate), value key and tie key
template <int KIND>   // 0: uint32 ascending, 1: f64 ascending, 2: f64 descending
__device__ __forceinline__ unsigned candidate(const State &s, size_t n, size_t t, const unsigned *__restrict__ rows, const unsigned *__restrict__ cols,
                                              const void *__restrict__ value, const double *__restrict__ e_mask, double e_max,
                                              unsigned long long &key, unsigned long long &tie)
{
    const unsigned r = rows[t], c = cols[t];
    if (r == c || (size_t)r >= n || (size_t)c >= n) return NO_VERTEX;      // not a pair of this state: skipped
    if (e_mask && !(e_max >= e_mask[t])) return NO_VERTEX;                   // the -K test (tracs/distance.py:222): NaN fails
    const long long dr = s.days[r], dc = s.days[c];
    if (dr == dc) return NO_VERTEX;                                          // same day: never each other's source
    const unsigned later = dr > dc ? r : c, earlier = dr > dc ? c : r;
    const unsigned long long gap = (unsigned long long)(dr > dc ? dr - dc : dc - dr);      // <= 2^32 - 1: 64-bit, pre-1970 days too
    if (KIND == 0) key = static_cast<const unsigned *>(value)[t];
    else if (KIND == 1) key = f64_key_up(static_cast<const double *>(value)[t]);
    else key = f64_key_down(static_cast<const double *>(value)[t]);
    tie = (gap << 32) | earlier;
    return later;
}

__global__ __launch_bounds__(256) void anc_init_kernel(State s, size_t n, const int *__restrict__ days)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) {
        s.days[v] = days[v];
        s.bv[v] = KEY_NONE; s.bt[v] = KEY_NONE; s.cv[v] = KEY_NONE; s.win[v] = NO_VERTEX;
        s.pa[v] = NO_VERTEX; s.val.d[v] = 0; s.val.nn[v] = 0; s.val.f[v] = 0; s.val.p[v] = 0.0; s.val.e[v] = 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { s.hdr->n = n; s.hdr->taken = 0; s.hdr->links = 0; }
}

// Pass 1: every candidate's later endpoint takes its value key; the candidates are counted
template <int KIND>
__global__ __launch_bounds__(256) void anc_pass1_kernel(State s, size_t n, size_t m, const unsigned *__restrict__ rows, const unsigned *__restrict__ cols,
                                                        const void *__restrict__ value, const double *__restrict__ e_mask, double e_max)
{
    const int lane = threadIdx.x & 63;
    unsigned long long cnt = 0;
    for (size_t base = (size_t)blockIdx.x * 256; base < m; base += (size_t)gridDim.x * 256) {
        const size_t t = base + threadIdx.x;
        unsigned tgt = NO_VERTEX;
        unsigned long long key = KEY_NONE, tie = KEY_NONE;
        if (t < m) tgt = candidate<KIND>(s, n, t, rows, cols, value, e_mask, e_max, key, tie);
        if (tgt == NO_VERTEX) key = KEY_NONE; else cnt++;
        wave_min_into(s.bv, key, tgt, lane);
    }
    wave_add_into(&s.hdr->taken, cnt, lane);
}

// Settle: a vertex whose value key this update lowered forgets the tie key of its stored winner; every vertex forgets the last batch's index
__global__ __launch_bounds__(256) void anc_settle_kernel(State s, size_t n)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) {
        if (s.bv[v] != s.cv[v]) s.bt[v] = KEY_NONE;
        s.win[v] = NO_VERTEX;
    }
}

// Pass 2: among the candidates that tie a vertex's value key, the vertex takes the smallest gap << 32 | a
template <int KIND>
__global__ __launch_bounds__(256) void anc_pass2_kernel(State s, size_t n, size_t m, const unsigned *__restrict__ rows, const unsigned *__restrict__ cols,
                                                        const void *__restrict__ value, const double *__restrict__ e_mask, double e_max)
{
    const int lane = threadIdx.x & 63;
    for (size_t base = (size_t)blockIdx.x * 256; base < m; base += (size_t)gridDim.x * 256) {
        const size_t t = base + threadIdx.x;
        unsigned tgt = NO_VERTEX;
        unsigned long long key = KEY_NONE, tie = KEY_NONE;
        if (t < m) tgt = candidate<KIND>(s, n, t, rows, cols, value, e_mask, e_max, key, tie);
        if (tgt != NO_VERTEX && key != s.bv[tgt]) tgt = NO_VERTEX;
        if (tgt == NO_VERTEX) tie = KEY_NONE;
        wave_min_into(s.bt, tie, tgt, lane);
    }
}

// Pass 3: the candidate that holds both of a vertex's keys records its index in the batch
template <int KIND>
__global__ __launch_bounds__(256) void anc_pass3_kernel(State s, size_t n, size_t m, const unsigned *__restrict__ rows, const unsigned *__restrict__ cols,
                                                        const void *__restrict__ value, const double *__restrict__ e_mask, double e_max)
{
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < m; t += (size_t)gridDim.x * 256) {
        unsigned long long key = KEY_NONE, tie = KEY_NONE;
        const unsigned tgt = candidate<KIND>(s, n, t, rows, cols, value, e_mask, e_max, key, tie);
        if (tgt != NO_VERTEX && key == s.bv[tgt] && tie == s.bt[tgt]) s.win[tgt] = (unsigned)t;
    }
}

// Gather: a vertex won by a pair of this batch takes its parent and the pair's values; its committed value key follows
__global__ __launch_bounds__(256) void anc_gather_kernel(State s, size_t n, size_t m, PairColumns batch)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) {
        const size_t w = s.win[v];
        if (w >= m) continue;                                     // (NO_VERTEX: the stored winner stays)
        s.pa[v] = (unsigned)(s.bt[v] & 0xffffffffull);
        take_columns(s.val, v, batch, w);
        s.cv[v] = s.bv[v];
    }
}

// Emit, step 1: the sort key of every vertex's link (roots: KEY_NONE, sorted behind every link), the link count, and the first hop and
// generation of the pointer doubling (a root points at itself, generation 0)
__global__ __launch_bounds__(256) void anc_links_kernel(State s, size_t n)
{
    const int lane = threadIdx.x & 63;
    unsigned long long cnt = 0;
    for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {
        const size_t v = base + threadIdx.x;
        if (v >= n) continue;
        const unsigned p = s.pa[v];
        const bool link = p != NO_VERTEX && (size_t)p < n;
        const unsigned lo = (unsigned)v < p ? (unsigned)v : p, hi = (unsigned)v < p ? p : (unsigned)v;
        s.keys[v] = link ? ((unsigned long long)lo << 32) | hi : KEY_NONE;
        s.idx[v] = (unsigned)v;
        s.hop[v] = link ? p : (unsigned)v;
        s.gen[v] = link ? 1u : 0u;
        cnt += link ? 1 : 0;
    }
    wave_add_into(&s.hdr->links, cnt, lane);
}

// row k of the output: vertex order[k] and its parent, the smaller index first
__global__ __launch_bounds__(256) void anc_emit_kernel(State s, size_t n_links, const unsigned *__restrict__ order, unsigned *rows, unsigned *cols,
                                                       PairColumns out)
{
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n_links; k += (size_t)gridDim.x * 256) {
        const unsigned v = order[k], a = s.pa[v];
        if (rows) rows[k] = v < a ? v : a;
        if (cols) cols[k] = v < a ? a : v;
        emit_columns(out, k, s.val, v);
    }
}

// One round of pointer doubling, from one buffer into the other (no vertex is read and written in one launch): after round k a
// vertex's hop is its ancestor 2^k links up, or its root
__global__ __launch_bounds__(256) void anc_double_kernel(size_t n, const unsigned *__restrict__ hop_in, const unsigned *__restrict__ gen_in,
                                                         unsigned *__restrict__ hop_out, unsigned *__restrict__ gen_out)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) {
        const unsigned h = hop_in[v];
        gen_out[v] = gen_in[v] + gen_in[h];
        hop_out[v] = hop_in[h];
    }
}

}  // namespace

extern "C" {

size_t tracs_anc_state_bytes(size_t n) { return arena_bytes<State>(n); }

int tracs_anc_init(void *state, size_t n, const int32_t *days_device, void *stream_)
{
    if (!state) { set_error("tracs_anc_init: NULL state"); return TRACS_E_ARG; }
    if (n && !days_device) { set_error("tracs_anc_init: NULL days"); return TRACS_E_ARG; }
    if (n >= (1ull << 31)) { set_error("tracs_anc_init: more than 2^31 vertices"); return TRACS_E_ARG; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceCall guard(stream);
    State s(state, n);
    hipLaunchKernelGGL(anc_init_kernel, dim3(grid_for(n, SELECT_BLOCKS)), dim3(256), 0, stream, s, n, days_device);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

int tracs_anc_update_coo(void *state, size_t n, size_t m, const uint32_t *rows, const uint32_t *cols, const void *value, int value_kind,
                         const double *e_mask, double e_max, const uint32_t *d, const uint32_t *nn, const uint32_t *filt,
                         const double *p, const double *e, uint64_t *n_taken, void *stream_)
{
    if (n_taken) *n_taken = 0;
    if (!state) { set_error("tracs_anc_update_coo: NULL state"); return TRACS_E_ARG; }
    if (value_kind < 0 || value_kind > 2) {
        set_error("tracs_anc_update_coo: value_kind must be 0 (uint32 ascending), 1 (f64 ascending) or 2 (f64 descending)");
        return TRACS_E_ARG;
    }
    if (m && (!rows || !cols || !value)) { set_error("tracs_anc_update_coo: NULL pair array"); return TRACS_E_ARG; }
    if (m >= 0xFFFFFFFFull) { set_error("tracs_anc_update_coo: more than 2^32 - 2 pairs in one batch"); return TRACS_E_ARG; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceCall guard(stream);
    State s(state, n);
    Hdr h{};
    int rc;
    if ((rc = read_state_header(s.hdr, n, "tracs_anc_update_coo", stream, &h))) return rc;
    if (m == 0 || n < 2) return TRACS_OK;
    const unsigned nb = grid_for(n, SELECT_BLOCKS), eb = grid_for(m, SELECT_BLOCKS);
    TRACS_HIP_CHECK(hipMemsetAsync(&s.hdr->taken, 0, 8, stream));
    auto pass = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(eb), dim3(256), 0, stream, s, n, m, rows, cols, value, e_mask, e_max); };
    auto passes = [&](auto pass1, auto pass2, auto pass3) {
        pass(pass1);
        hipLaunchKernelGGL(anc_settle_kernel, dim3(nb), dim3(256), 0, stream, s, n);
        pass(pass2);
        pass(pass3);
    };
    if (value_kind == 0) passes(anc_pass1_kernel<0>, anc_pass2_kernel<0>, anc_pass3_kernel<0>);
    else if (value_kind == 1) passes(anc_pass1_kernel<1>, anc_pass2_kernel<1>, anc_pass3_kernel<1>);
    else passes(anc_pass1_kernel<2>, anc_pass2_kernel<2>, anc_pass3_kernel<2>);
    hipLaunchKernelGGL(anc_gather_kernel, dim3(nb), dim3(256), 0, stream, s, n, m, batch_columns(d, nn, filt, p, e));
    TRACS_HIP_CHECK(hipGetLastError());
    if (n_taken) {
        unsigned long long taken = 0;
        TRACS_HIP_CHECK(hipMemcpyAsync(&taken, &s.hdr->taken, 8, hipMemcpyDeviceToHost, stream));
        TRACS_HIP_CHECK(hipStreamSynchronize(stream));
        *n_taken = taken;
    }
    return TRACS_OK;
}

int tracs_anc_emit(void *state, size_t n, size_t *n_links, uint32_t *rows, uint32_t *cols, uint32_t *d, uint32_t *nn, uint32_t *filt,
                   double *p, double *e, uint32_t *parent, uint32_t *root, uint32_t *generation, void *stream_)
{
    if (!state || !n_links) { set_error("tracs_anc_emit: NULL argument"); return TRACS_E_ARG; }
    *n_links = 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceCall guard(stream);
    State s(state, n);
    Hdr h{};
    int rc;
    if ((rc = read_state_header(s.hdr, n, "tracs_anc_emit", stream, &h))) return rc;
    if (n == 0) return TRACS_OK;
    const unsigned nb = grid_for(n, SELECT_BLOCKS);
    TRACS_HIP_CHECK(hipMemsetAsync(&s.hdr->links, 0, 8, stream));
    hipLaunchKernelGGL(anc_links_kernel, dim3(nb), dim3(256), 0, stream, s, n);
    TRACS_HIP_CHECK(hipGetLastError());
    unsigned long long links = 0;
    TRACS_HIP_CHECK(hipMemcpyAsync(&links, &s.hdr->links, 8, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    const size_t nl = std::min<size_t>((size_t)links, n);
    *n_links = nl;
    if (nl && (rows || cols || d || nn || filt || p || e)) {
        // every vertex's key is sorted (roots carry KEY_NONE and end up behind the links); the first nl entries are the links in (i, j) order
        if ((rc = sort_by_pair_key(s.keys, s.idx, n, s.cap, WS_ANC_SORT_TMP, stream))) return rc;
        hipLaunchKernelGGL(anc_emit_kernel, dim3(grid_for(nl, SELECT_BLOCKS)), dim3(256), 0, stream, s, nl, s.idx + s.cap, rows, cols,
                           PairColumns{d, nn, filt, p, e});
        TRACS_HIP_CHECK(hipGetLastError());
    }
    if (parent) TRACS_HIP_CHECK(hipMemcpyAsync(parent, s.pa, n * 4, hipMemcpyDeviceToDevice, stream));
    if (root || generation) {
        int rounds = 0;
        while (((size_t)1 << rounds) < n) rounds++;              // ceil(log2 n): 2^rounds >= n > the longest chain's n - 1 links
        int cur = 0;
        for (int k = 0; k < rounds; k++, cur ^= 1)
            hipLaunchKernelGGL(anc_double_kernel, dim3(nb), dim3(256), 0, stream, n, s.hop + cur * s.cap, s.gen + cur * s.cap,
                               s.hop + (cur ^ 1) * s.cap, s.gen + (cur ^ 1) * s.cap);
        TRACS_HIP_CHECK(hipGetLastError());
        if (root) TRACS_HIP_CHECK(hipMemcpyAsync(root, s.hop + cur * s.cap, n * 4, hipMemcpyDeviceToDevice, stream));
        if (generation) TRACS_HIP_CHECK(hipMemcpyAsync(generation, s.gen + cur * s.cap, n * 4, hipMemcpyDeviceToDevice, stream));
    }
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    return TRACS_OK;
}

}  // extern "C"
