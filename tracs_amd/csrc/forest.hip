// forest.hip -- minimum spanning forest of the eligible pairs (tracs_msf_*, include/tracs_hip.h).
//
// Edges are ordered by (weight key, i, j) with i < j the pair's sample indices: a strict total order, so the forest is unique.  The
// weight key is order-preserving in 64 bits: a uint32 weight as is; an f64 weight through f64_key_up (pair_select.h).  A pair's (i, j) is a second 64-bit key, i << 32 | j: (weight, i, j) does not fit in 64 bits, so every
// minimum is taken in two steps, the weight first, then (i, j) among the edges that tie on it.
//
// State: the running forest F (at most n - 1 edges, each with the values its CSV row is written with) and per-vertex scratch.  An
// update with a batch B replaces F by MSF(F u B): by the cycle property no edge outside MSF(F) can be in MSF(F u B), so the result
// is MSF of everything offered so far, whatever the batch split or order.  The update is Boruvka on F u B:
//   pass 1   per live edge: both endpoint components take the edge's weight key (atomicMin); the edges whose endpoints lie in one
//            component are compacted away, the rest go to the other half of a ping-pong buffer (one atomic per wave for the slot)
//   pass 2   per live edge that ties its component's minimum weight: the component takes its (i, j) (atomicMin)
//   pass 3   the edge that won a component records its index
//   hook     per component root with a winner: the edge goes into the new forest and the two components are joined, the larger
//            root under the smaller (pair_select.h's union-find, as csrc/cluster.hip); a mutual pick of one edge (the only cycle a strict total order
//            lets Boruvka form) is counted once, by the smaller root
//   flatten  every vertex's component label <- its root
// Atomics are reduced across the wave first (wave_min_into, pair_select.h): in row-major COO consecutive edges share a row, so a
// segmented minimum over runs of one component leaves one atomic per run.  The host reads one word per round (the live edge count)
// and stops when it is 0.
// Emit sorts the forest by (i, j) (rocprim radix sort) and gathers the row values.
#include "common.h"
#include "pair_select.h"

using namespace tracs;

namespace {

struct Hdr {
    unsigned long long nf;          // forest edges
    unsigned long long nf_new;      // forest edges chosen by the running update
    unsigned long long live;        // live edges compacted by the last pass 1
    unsigned long long n;           // vertices the state was initialised for
};

// State: header, then the forest (capacity max(n, 1): endpoints, weight key, values), then per-vertex scratch
struct State {
    Hdr *hdr;
    unsigned *fi, *fj;
    unsigned long long *fw;
    PairColumns val;
    int *comp, *par;
    unsigned long long *bw, *bij;
    unsigned *win;
    State(void *base, size_t n, size_t *bytes = nullptr)
    {
        const size_t cap = std::max<size_t>(n, 1);
        Arena a(base, bytes);
        hdr = reinterpret_cast<Hdr *>(a.take<char>(64));
        fi = a.take<unsigned>(cap); fj = a.take<unsigned>(cap); fw = a.take<unsigned long long>(cap);
        val.d = a.take<unsigned>(cap); val.nn = a.take<unsigned>(cap); val.f = a.take<unsigned>(cap);
        val.p = a.take<double>(cap); val.e = a.take<double>(cap);
        comp = a.take<int>(cap); par = a.take<int>(cap); bw = a.take<unsigned long long>(cap); bij = a.take<unsigned long long>(cap);
        win = a.take<unsigned>(cap);
    }
};

// the working edge list of one round (struct of arrays): endpoints i < j, weight key, index into F u B (< nf: F, else B)
struct Work {
    unsigned *i, *j, *src; unsigned long long *w;
    Work(void *base, size_t m, size_t *bytes = nullptr)
    {
        Arena a(base, bytes);
        i = a.take<unsigned>(m); j = a.take<unsigned>(m); src = a.take<unsigned>(m); w = a.take<unsigned long long>(m);
    }
};

// the new forest: fsrc[k] indexes F (< nf) or the batch (>= nf); its values gathered into the temporary forest `t` (capacity n)
struct Forest {
    unsigned *i, *j; unsigned long long *w; PairColumns val;
    Forest(void *base, size_t n, size_t *bytes = nullptr)
    {
        Arena a(base, bytes);
        w = a.take<unsigned long long>(n); val.p = a.take<double>(n); val.e = a.take<double>(n);
        i = a.take<unsigned>(n); j = a.take<unsigned>(n); val.d = a.take<unsigned>(n); val.nn = a.take<unsigned>(n); val.f = a.take<unsigned>(n);
    }
};

__global__ __launch_bounds__(256) void msf_init_kernel(State s, size_t n)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) { s.comp[v] = (int)v; s.par[v] = (int)v; }
    if (blockIdx.x == 0 && threadIdx.x == 0) { s.hdr->nf_new = 0; s.hdr->live = 0; }
}

__global__ __launch_bounds__(256) void msf_reset_kernel(State s, size_t n)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) { s.bw[v] = KEY_NONE; s.bij[v] = KEY_NONE; }
}

// Pass 1.  first != 0: the edges are F (index < nf) followed by the batch (rows, cols, weight, mask); else the working list `in`.
// Live edges go to `out` (slot from hdr->live); both endpoint components take the edge's weight key.
template <int KIND>   // 0: uint32 weights, 1: f64 weights (first round only)
__global__ __launch_bounds__(256) void msf_pass1_kernel(State s, size_t n, int first, size_t n_in, Work in, const unsigned *__restrict__ rows,
                                                        const unsigned *__restrict__ cols, const void *__restrict__ weight,
                                                        const double *__restrict__ e_mask, double e_max, Work out)
{
    const int lane = threadIdx.x & 63;
    const size_t nf = first ? (size_t)s.hdr->nf : 0;
    for (size_t base = (size_t)blockIdx.x * 256; base < n_in; base += (size_t)gridDim.x * 256) {
        const size_t e = base + threadIdx.x;
        unsigned a = 0, b = 0, src = 0;
        unsigned long long w = KEY_NONE;
        if (e < n_in) {
            if (!first) { a = in.i[e]; b = in.j[e]; w = in.w[e]; src = in.src[e]; }
            else if (e < nf) { a = s.fi[e]; b = s.fj[e]; w = s.fw[e]; src = (unsigned)e; }
            else {
                const size_t t = e - nf;
                const unsigned r = rows[t], c = cols[t];
                a = r < c ? r : c; b = r < c ? c : r; src = (unsigned)e;
                if (KIND == 0) w = static_cast<const unsigned *>(weight)[t];
                else w = f64_key_up(static_cast<const double *>(weight)[t]);
                if (e_mask && !(e_max >= e_mask[t])) w = KEY_NONE;     // the -K test (tracs/distance.py:222): NaN fails
                if (a == b || (size_t)b >= n) w = KEY_NONE;             // not an edge of this state: skipped
            }
        }
        unsigned ca = NO_VERTEX, cb = NO_VERTEX;
        if (w != KEY_NONE) { ca = (unsigned)s.comp[a]; cb = (unsigned)s.comp[b]; }
        const bool live = w != KEY_NONE && ca != cb;
        if (!live) { w = KEY_NONE; ca = cb = NO_VERTEX; }
        // compaction: one slot reservation per wave
        const unsigned long long mask = __ballot(live);
        unsigned long long slot0 = 0;
        if (lane == 0 && mask) slot0 = atomicAdd(&s.hdr->live, (unsigned long long)__popcll(mask));
        slot0 = __shfl(slot0, 0, 64);
        if (live) {
            const size_t at = (size_t)slot0 + (size_t)__popcll(mask & ((1ull << lane) - 1ull));
            out.i[at] = a; out.j[at] = b; out.w[at] = w; out.src[at] = src;
        }
        wave_min_into(s.bw, w, ca, lane);
        wave_min_into(s.bw, w, cb, lane);
    }
}

// Pass 2: among the live edges that tie a component's minimum weight, the component takes the smallest (i, j)
__global__ __launch_bounds__(256) void msf_pass2_kernel(State s, size_t n_live, Work in)
{
    const int lane = threadIdx.x & 63;
    for (size_t base = (size_t)blockIdx.x * 256; base < n_live; base += (size_t)gridDim.x * 256) {
        const size_t e = base + threadIdx.x;
        unsigned ca = NO_VERTEX, cb = NO_VERTEX;
        unsigned long long ka = KEY_NONE, kb = KEY_NONE;
        if (e < n_live) {
            const unsigned a = in.i[e], b = in.j[e];
            const unsigned long long w = in.w[e], ij = ((unsigned long long)a << 32) | b;
            ca = (unsigned)s.comp[a]; cb = (unsigned)s.comp[b];
            if (w == s.bw[ca]) ka = ij; else ca = NO_VERTEX;
            if (w == s.bw[cb]) kb = ij; else cb = NO_VERTEX;
        }
        wave_min_into(s.bij, ka, ca, lane);
        wave_min_into(s.bij, kb, cb, lane);
    }
}

// Pass 3: the winning edge of each component records its index in F u B (unique: (i, j) is)
__global__ __launch_bounds__(256) void msf_pass3_kernel(State s, size_t n_live, Work in)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n_live; e += (size_t)gridDim.x * 256) {
        const unsigned a = in.i[e], b = in.j[e];
        const unsigned long long w = in.w[e], ij = ((unsigned long long)a << 32) | b;
        const int ca = s.comp[a], cb = s.comp[b];
        if (w == s.bw[ca] && ij == s.bij[ca]) s.win[ca] = in.src[e];
        if (w == s.bw[cb] && ij == s.bij[cb]) s.win[cb] = in.src[e];
    }
}

// Hook: each component root with a winner adds it to the new forest (a mutual pick once, by the smaller root) and joins the two
// components in the union-find `par` (larger root under the smaller; comp stays this round's snapshot)
__global__ __launch_bounds__(256) void msf_hook_kernel(State s, size_t n, unsigned *__restrict__ fsrc)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) {
        if (s.comp[v] != (int)v || s.bw[v] == KEY_NONE) continue;
        const unsigned long long ij = s.bij[v];
        const int ci = s.comp[(unsigned)(ij >> 32)], cj = s.comp[(unsigned)(ij & 0xffffffffu)];
        const int o = ci == (int)v ? cj : ci;
        const bool mutual = s.bw[o] == s.bw[v] && s.bij[o] == ij;
        if (mutual && (int)v > o) continue;
        const unsigned long long k = atomicAdd(&s.hdr->nf_new, 1ull);
        if (k < n) fsrc[k] = s.win[v];                           // (< n - 1 always: a forest; the bound only guards the buffer)
        int a = (int)v, b = o;
        for (;;) {
            a = uf_find(s.par, a);
            b = uf_find(s.par, b);
            if (a == b) break;
            if (a > b) { const int t = a; a = b; b = t; }
            const int old = atomicCAS(&s.par[b], b, a);
            if (old == b) break;
            b = old;
        }
    }
}

__global__ __launch_bounds__(256) void msf_flatten_kernel(State s, size_t n)
{
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) {
        int x = (int)v;
        for (int p = uf_load(&s.par[x]); p != x; p = uf_load(&s.par[x])) x = p;
        s.comp[v] = x;
        __hip_atomic_store(&s.par[v], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void msf_gather_kernel(State s, const unsigned *__restrict__ fsrc, const unsigned *__restrict__ rows,
                                                         const unsigned *__restrict__ cols, const void *__restrict__ weight, int kind,
                                                         PairColumns batch, Forest t, size_t n)
{
    const size_t nf = (size_t)s.hdr->nf, nf_new = std::min<size_t>((size_t)s.hdr->nf_new, n);
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < nf_new; k += (size_t)gridDim.x * 256) {
        const size_t q = fsrc[k];
        if (q < nf) {
            t.i[k] = s.fi[q]; t.j[k] = s.fj[q]; t.w[k] = s.fw[q];
            copy_columns(t.val, k, s.val, q);
        } else {
            const size_t b = q - nf;
            const unsigned r = rows[b], c = cols[b];
            t.i[k] = r < c ? r : c; t.j[k] = r < c ? c : r;
            t.w[k] = kind == 0 ? (unsigned long long)static_cast<const unsigned *>(weight)[b] : f64_key_up(static_cast<const double *>(weight)[b]);
            take_columns(t.val, k, batch, b);
        }
    }
}

__global__ __launch_bounds__(256) void msf_commit_kernel(State s, Forest t, size_t n)
{
    const size_t nf_new = std::min<size_t>((size_t)s.hdr->nf_new, n);
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < nf_new; k += (size_t)gridDim.x * 256) {
        s.fi[k] = t.i[k]; s.fj[k] = t.j[k]; s.fw[k] = t.w[k];
        copy_columns(s.val, k, t.val, k);
    }
}

__global__ void msf_count_kernel(State s, size_t n)
{
    if (threadIdx.x == 0) s.hdr->nf = std::min<size_t>((size_t)s.hdr->nf_new, n);
}

__global__ __launch_bounds__(256) void msf_sort_keys_kernel(State s, size_t nf, unsigned long long *__restrict__ keys, unsigned *__restrict__ idx)
{
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < nf; k += (size_t)gridDim.x * 256) {
        keys[k] = ((unsigned long long)s.fi[k] << 32) | s.fj[k];
        idx[k] = (unsigned)k;
    }
}

// row k of the output: the forest's edge order[k] with its stored endpoints
__global__ __launch_bounds__(256) void msf_emit_kernel(State s, size_t nf, const unsigned *__restrict__ order, unsigned *rows, unsigned *cols,
                                                       PairColumns out)
{
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < nf; k += (size_t)gridDim.x * 256) {
        const unsigned q = order[k];
        if (rows) rows[k] = s.fi[q];
        if (cols) cols[k] = s.fj[q];
        emit_columns(out, k, s.val, q);
    }
}

}  // namespace

extern "C" {

size_t tracs_msf_state_bytes(size_t n) { return arena_bytes<State>(n); }

int tracs_msf_init(void *state, size_t n, void *stream_)
{
    if (!state) { set_error("tracs_msf_init: NULL state"); return TRACS_E_ARG; }
    if (n >= (1ull << 31)) { set_error("tracs_msf_init: more than 2^31 vertices"); return TRACS_E_ARG; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceCall guard(stream);
    const Hdr h0{0, 0, 0, (unsigned long long)n};
    State s(state, n);
    TRACS_HIP_CHECK(hipMemcpyAsync(s.hdr, &h0, sizeof(h0), hipMemcpyHostToDevice, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));           // (h0 lives on this frame)
    return TRACS_OK;
}

int tracs_msf_update_coo(void *state, size_t n, size_t m, const uint32_t *rows, const uint32_t *cols, const void *weight, int weight_kind,
                         const double *e_mask, double e_max, const uint32_t *d, const uint32_t *nn, const uint32_t *filt,
                         const double *p, const double *e, uint64_t *n_taken, void *stream_)
{
    if (n_taken) *n_taken = 0;
    if (!state) { set_error("tracs_msf_update_coo: NULL state"); return TRACS_E_ARG; }
    if (weight_kind != 0 && weight_kind != 1) { set_error("tracs_msf_update_coo: weight_kind must be 0 (uint32) or 1 (f64)"); return TRACS_E_ARG; }
    if (m && (!rows || !cols || !weight)) { set_error("tracs_msf_update_coo: NULL edge array"); return TRACS_E_ARG; }
    if (m >= (1ull << 32)) { set_error("tracs_msf_update_coo: more than 2^32 - 1 edges in one batch"); return TRACS_E_ARG; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceCall guard(stream);
    State s(state, n);
    Hdr h{};
    int rc;
    if ((rc = read_state_header(s.hdr, n, "tracs_msf_update_coo", stream, &h))) return rc;
    const size_t nf = (size_t)h.nf, total = nf + m;
    if (total == 0 || n < 2) return TRACS_OK;
    if (total >= (1ull << 32)) { set_error("tracs_msf_update_coo: forest + batch exceed 2^32 - 1 edges"); return TRACS_E_ARG; }
    unsigned *fsrc;
    char *wb[2], *tb;
    if ((rc = workspace_get(WS_MSF_W0, arena_bytes<Work>(total), &wb[0]))) return rc;
    if ((rc = workspace_get(WS_MSF_W1, arena_bytes<Work>(total), &wb[1]))) return rc;
    Work w[2] = {Work(wb[0], total), Work(wb[1], total)};
    if ((rc = workspace_get(WS_MSF_FSRC, n, &fsrc))) return rc;
    const unsigned nb = grid_for(n, SELECT_BLOCKS);
    hipLaunchKernelGGL(msf_init_kernel, dim3(nb), dim3(256), 0, stream, s, n);
    size_t n_in = total;
    int cur = 0;
    for (int round = 0;; round++) {
        hipLaunchKernelGGL(msf_reset_kernel, dim3(nb), dim3(256), 0, stream, s, n);
        TRACS_HIP_CHECK(hipMemsetAsync(&s.hdr->live, 0, 8, stream));
        Work &out = w[cur ^ (round ? 1 : 0)];
        hipLaunchKernelGGL(weight_kind == 0 ? msf_pass1_kernel<0> : msf_pass1_kernel<1>, dim3(grid_for(n_in, SELECT_BLOCKS)), dim3(256), 0,
                           stream, s, n, round == 0 ? 1 : 0, n_in, w[cur], rows, cols, weight, e_mask, e_max, out);
        TRACS_HIP_CHECK(hipGetLastError());
        unsigned long long live = 0;                             // the one word per round
        TRACS_HIP_CHECK(hipMemcpyAsync(&live, &s.hdr->live, 8, hipMemcpyDeviceToHost, stream));
        TRACS_HIP_CHECK(hipStreamSynchronize(stream));
        if (round == 0 && n_taken) *n_taken = live - nf;         // F's edges are all live in round 0: the rest are the batch's eligible ones
        if (live == 0) break;
        if (round) cur ^= 1;                                     // round 0 read F u B and wrote w[cur]; later rounds ping-pong
        const unsigned eb = grid_for((size_t)live, SELECT_BLOCKS);
        hipLaunchKernelGGL(msf_pass2_kernel, dim3(eb), dim3(256), 0, stream, s, (size_t)live, w[cur]);
        hipLaunchKernelGGL(msf_pass3_kernel, dim3(eb), dim3(256), 0, stream, s, (size_t)live, w[cur]);
        hipLaunchKernelGGL(msf_hook_kernel, dim3(nb), dim3(256), 0, stream, s, n, fsrc);
        hipLaunchKernelGGL(msf_flatten_kernel, dim3(nb), dim3(256), 0, stream, s, n);
        TRACS_HIP_CHECK(hipGetLastError());
        n_in = (size_t)live;
    }
    // the new forest (< n edges): gather its values from F and the batch, then commit
    if ((rc = workspace_get(WS_MSF_FTMP, arena_bytes<Forest>(n), &tb))) return rc;
    const Forest t(tb, n);
    hipLaunchKernelGGL(msf_gather_kernel, dim3(nb), dim3(256), 0, stream, s, fsrc, rows, cols, weight, weight_kind,
                       batch_columns(d, nn, filt, p, e), t, n);
    hipLaunchKernelGGL(msf_commit_kernel, dim3(nb), dim3(256), 0, stream, s, t, n);
    hipLaunchKernelGGL(msf_count_kernel, dim3(1), dim3(64), 0, stream, s, n);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

int tracs_msf_emit(void *state, size_t n, size_t *n_edges, uint32_t *rows, uint32_t *cols, uint32_t *d, uint32_t *nn, uint32_t *filt,
                   double *p, double *e, void *stream_)
{
    if (!state || !n_edges) { set_error("tracs_msf_emit: NULL argument"); return TRACS_E_ARG; }
    *n_edges = 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceCall guard(stream);
    State s(state, n);
    Hdr h{};
    int rc;
    if ((rc = read_state_header(s.hdr, n, "tracs_msf_emit", stream, &h))) return rc;
    const size_t nf = std::min<size_t>((size_t)h.nf, n);
    *n_edges = nf;
    if (nf == 0) return TRACS_OK;
    unsigned long long *keys;
    unsigned *idx;
    if ((rc = workspace_get(WS_MSF_SORT_KEYS, nf * 2, &keys))) return rc;
    if ((rc = workspace_get(WS_MSF_SORT_IDX, nf * 2, &idx))) return rc;
    hipLaunchKernelGGL(msf_sort_keys_kernel, dim3(grid_for(nf, SELECT_BLOCKS)), dim3(256), 0, stream, s, nf, keys, idx);
    TRACS_HIP_CHECK(hipGetLastError());
    if ((rc = sort_by_pair_key(keys, idx, nf, nf, WS_MSF_SORT_TMP, stream))) return rc;
    hipLaunchKernelGGL(msf_emit_kernel, dim3(grid_for(nf, SELECT_BLOCKS)), dim3(256), 0, stream, s, nf, idx + nf, rows, cols,
                       PairColumns{d, nn, filt, p, e});
    TRACS_HIP_CHECK(hipGetLastError());
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    return TRACS_OK;
}

}  // extern "C"
