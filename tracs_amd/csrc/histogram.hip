// histogram.hip -- running histogram of pair values over the dense pair panels (tracs_hist_*, include/tracs_hip.h).
//
// A pair (i, j) with value v is counted in bin v of one of three classes: 0 within (both samples grouped, equal labels), 1 between
// (both grouped, labels differ), 2 ungrouped (a label < 0, or no labels at all).  Counts are 64-bit and exact: the result is a sum,
// so it does not depend on panel splits, launch order or the route a cell took below.
//
// State (caller-owned device buffer, hist_state_bytes(n_bins)):
//   header  8 x uint64: [0] cells with v >= n_bins (never dropped silently: tracs_hist_emit fails on them), [1..3] cells counted by
//           each route (tracs_debug_hist_routes), rest 0
//   bins    uint64[3][n_bins], class-major
//   chunks  int64[n_chunks + 1]: scratch of tracs_hist_emit (non-empty bins per chunk of 1024 bins, then their exclusive offsets)
//
// Counting.  A workgroup (four waves) keeps HIST_W tagged 32-bit bins per class in LDS: value v lives in slot v % HIST_W while the
// slot's tag is v / HIST_W.  The first value that reaches a free slot claims it (compare-and-swap on the tag); a value that finds
// its slot held by another tag goes to the 64-bit global bins directly.  So the window is not a range: a panel with d ~ 0 and
// d ~ 20 000 keeps both modes in LDS, and only values that collide modulo HIST_W leave it.  The LDS bins are flushed -- one global
// atomic per non-empty (slot, class) -- at the end and before a workgroup can have counted 2^32 cells since its last flush.
// Routes, per 64 cells of a wave:
//   1 combined  the (value, class) of the first pending lane is probed: when it covers at least HIST_HOT of the pending lanes
//               (identical isolates: all 64), its lanes are counted by ONE LDS add of their number (ballot + popcount), at most
//               HIST_ROUNDS times; a probe that finds a rare value moves on to the first lane with another value, HIST_COLD_TRIES
//               times at most, so a hot value behind an odd first cell is still found;
//   2 lds       the other lanes add 1 each to their slot;
//   3 global    lanes whose slot carries another tag: atomicAdd on the 64-bit bin.
// The panel is read once, coalesced: a wave per row, 4 x 64 consecutive cells per step, and the columns' labels as one int32 load
// per cell from an array of n labels that stays in L2; the row's label is wave-uniform.
#include "common.h"
#include "scan_kernels.h"
#include "debug_api.h"

#include <algorithm>
#include <cstdlib>

namespace {

constexpr int HIST_W = 1024;                 // LDS slots per class
constexpr int HIST_HOT = 16;                 // lanes of one (value, class) that make a combined add worth its ballot
constexpr int HIST_ROUNDS = 3;               // combined adds per 64 cells at most (one per class when every pair has one value)
#ifndef HIST_COLD_TRIES
#define HIST_COLD_TRIES 2                    // probes per 64 cells that may find a rare value before the wave stops probing
#endif
constexpr unsigned HIST_EMPTY = 0xFFFFFFFFu;
constexpr int HIST_HEADER = 8;               // uint64 words
constexpr int HIST_CHUNK = 1024;             // bins per workgroup of the emit kernels

typedef unsigned long long u64;

inline size_t hist_chunks(size_t n_bins) { return (n_bins + HIST_CHUNK - 1) / HIST_CHUNK; }
inline size_t hist_bytes(size_t n_bins) { return 8 * (HIST_HEADER + 3 * n_bins + hist_chunks(n_bins) + 1); }
inline u64 *hist_bins(void *state) { return static_cast<u64 *>(state) + HIST_HEADER; }
inline long long *hist_chunk_words(void *state, size_t n_bins) { return reinterpret_cast<long long *>(hist_bins(state) + 3 * n_bins); }

// The workgroup's LDS bins and the per-lane route counters.  NCLS: 3 with labels, 1 without (everything is class 2).
template <int NCLS>
struct Counter {
    unsigned *tag;            // [HIST_W]
    unsigned *cnt;            // [NCLS][HIST_W]
    u64 *header, *bins;
    unsigned n_bins;
    u64 c_over = 0, c_comb = 0, c_lds = 0, c_glob = 0;

    __device__ __forceinline__ unsigned *slot_word(int cls, unsigned slot) const
    {
        return cnt + (NCLS == 1 ? 0 : cls) * HIST_W + slot;
    }

    __device__ void clear()
    {
        for (int t = threadIdx.x; t < HIST_W; t += blockDim.x) tag[t] = HIST_EMPTY;
        for (int t = threadIdx.x; t < NCLS * HIST_W; t += blockDim.x) cnt[t] = 0u;
    }

    // does slot v % HIST_W belong to v (claiming it when it is free)?  The plain read races with another wave's compare-and-swap, which
    // is harmless: between two barriers a tag only ever goes from HIST_EMPTY to one value, so a tag read as taken is final, and a
    // stale HIST_EMPTY is settled by the compare-and-swap's return value.
    __device__ __forceinline__ bool owns(unsigned v)
    {
        const unsigned slot = v % HIST_W, hi = v / HIST_W;
        unsigned t = tag[slot];
        if (t == HIST_EMPTY) {
            t = atomicCAS(&tag[slot], HIST_EMPTY, hi);
            if (t == HIST_EMPTY) t = hi;
        }
        return t == hi;
    }

    // 64 cells, one per lane (valid: the lane has one).  Every lane of the wave calls it.
    __device__ __forceinline__ void add(unsigned v, int cls, bool valid, int lane)
    {
        if (valid && v >= n_bins) { c_over++; valid = false; }
        u64 pending = __ballot(valid);                               // lanes whose value has not been probed
        const unsigned key_cls = NCLS == 1 ? 0u : (unsigned)cls;
        for (int round = 0, cold = 0; round < HIST_ROUNDS && cold < HIST_COLD_TRIES && pending; ) {      // all of it wave-uniform
            const int lead = __ffsll((long long)pending) - 1;
            const unsigned v0 = __shfl(v, lead, 64), k0 = __shfl(key_cls, lead, 64);
            const u64 same = __ballot(valid && v == v0 && key_cls == k0);
            const int m = __popcll(same);
            pending &= ~same;
            if (m < HIST_HOT) { cold++; continue; }                  // a rare value: its lanes take the per-lane routes below
            round++;
            if (lane == lead) {
                if (owns(v0)) atomicAdd(slot_word((int)k0, v0 % HIST_W), (unsigned)m);
                else atomicAdd(&bins[(size_t)(NCLS == 1 ? 2 : k0) * n_bins + v0], (u64)m);
                c_comb += (u64)m;
            }
            if (same >> lane & 1) valid = false;
        }
        if (valid) {
            if (owns(v)) {
                atomicAdd(slot_word(cls, v % HIST_W), 1u);
                c_lds++;
            } else {
                atomicAdd(&bins[(size_t)(NCLS == 1 ? 2 : cls) * n_bins + v], (u64)1);
                c_glob++;
            }
        }
    }

    // LDS bins -> global bins, and the LDS bins empty again.  The whole workgroup calls it.
    __device__ void flush()
    {
        __syncthreads();
        for (int s = threadIdx.x; s < HIST_W; s += blockDim.x) {
            const unsigned t = tag[s];
            if (t == HIST_EMPTY) continue;
            const size_t v = (size_t)t * HIST_W + s;
#pragma unroll
            for (int c = 0; c < NCLS; c++) {
                unsigned *w = slot_word(c, s);
                const u64 sum = *w;
                *w = 0u;
                if (sum) atomicAdd(&bins[(size_t)(NCLS == 1 ? 2 : c) * n_bins + v], sum);
            }
            tag[s] = HIST_EMPTY;
        }
        __syncthreads();
    }

    // the route counters of this wave -> header.  Every lane of the wave calls it.
    __device__ void finish(int lane)
    {
        auto total = [&](u64 c, int word) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if (lane == 0 && c) atomicAdd(&header[word], c);
        };
        total(c_over, 0);
        total(c_comb, 1);
        total(c_lds, 2);
        total(c_glob, 3);
    }
};

template <int NCLS>
__device__ __forceinline__ int pair_class(int gi, int gj)
{
    if (NCLS == 1) return 2;
    return (gi < 0 || gj < 0) ? 2 : (gi == gj ? 0 : 1);
}

// Wave w of workgroup b takes the panel rows row_begin + 4 * (b + k * gridDim.x) + w, k = 0, 1, ...; every `flush_every` steps k the
// workgroup flushes (4 rows of at most n cells per step: flush_every * 4 * n < 2^32).
template <int NCLS>
__global__ __launch_bounds__(256) void hist_panel_kernel(const unsigned *__restrict__ dist, size_t ld, unsigned n, unsigned row_begin,
                                                         unsigned row_end, unsigned col_begin, unsigned thr, const int *__restrict__ group,
                                                         u64 *__restrict__ state, unsigned n_bins, unsigned flush_every)
{
    __shared__ unsigned tag[HIST_W];
    __shared__ unsigned cnt[NCLS * HIST_W];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    Counter<NCLS> C;
    C.tag = tag; C.cnt = cnt; C.header = state; C.bins = state + HIST_HEADER; C.n_bins = n_bins;
    C.clear();
    __syncthreads();
    const unsigned steps = (row_end - row_begin + 4 * gridDim.x - 1) / (4 * gridDim.x);       // the same for every workgroup
    for (unsigned k = 0; k < steps; k++) {
        const u64 i64 = (u64)row_begin + 4ull * ((u64)blockIdx.x + (u64)k * gridDim.x) + w;
        if (i64 < row_end) {
            const unsigned i = (unsigned)i64;
            const unsigned *row = dist + (size_t)i * ld;
            const int gi = NCLS == 1 ? 0 : group[i];
            for (unsigned j0 = max(col_begin, i + 1); j0 < n; j0 += 256) {
                unsigned v[4];
                int g[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const unsigned j = j0 + 64 * u + lane;
                    v[u] = j < n ? row[j] : 0xFFFFFFFFu;
                    g[u] = (NCLS != 1 && j < n) ? group[j] : -1;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const unsigned j = j0 + 64 * u + lane;
                    if (j0 + 64 * u >= n) break;                          // uniform
                    C.add(v[u], pair_class<NCLS>(gi, g[u]), j < n && v[u] <= thr, lane);
                }
            }
        }
        if ((k + 1) % flush_every == 0 && k + 1 < steps) C.flush();
    }
    C.flush();
    C.finish(lane);
}

// The same for m listed pairs: thread t of the grid takes pairs t, t + threads, ...
template <int NCLS>
__global__ __launch_bounds__(256) void hist_coo_kernel(const unsigned *__restrict__ rows, const unsigned *__restrict__ cols,
                                                       const unsigned *__restrict__ val, size_t m, const int *__restrict__ group,
                                                       u64 *__restrict__ state, unsigned n_bins)
{
    __shared__ unsigned tag[HIST_W];
    __shared__ unsigned cnt[NCLS * HIST_W];
    const int lane = threadIdx.x & 63;
    Counter<NCLS> C;
    C.tag = tag; C.cnt = cnt; C.header = state; C.bins = state + HIST_HEADER; C.n_bins = n_bins;
    C.clear();
    __syncthreads();
    const size_t threads = (size_t)gridDim.x * 256;
    const size_t steps = (m + threads - 1) / threads;                                           // the same for every workgroup
    for (size_t k = 0; k < steps; k++) {
        const size_t t = k * threads + (size_t)blockIdx.x * 256 + threadIdx.x;
        const bool valid = t < m;
        const unsigned v = valid ? val[t] : 0u;
        const int cls = (NCLS != 1 && valid) ? pair_class<NCLS>(group[rows[t]], group[cols[t]]) : 2;
        C.add(v, cls, valid, lane);
        if ((k + 1) % (1u << 20) == 0 && k + 1 < steps) C.flush();                             // 2^28 cells per workgroup and flush
    }
    C.flush();
    C.finish(lane);
}

__device__ __forceinline__ bool bin_used(const u64 *bins, size_t n_bins, size_t b)
{
    return b < n_bins && (bins[b] | bins[n_bins + b] | bins[2 * n_bins + b]) != 0;
}

// non-empty bins of each chunk of HIST_CHUNK bins
__global__ __launch_bounds__(256) void hist_count_kernel(const u64 *__restrict__ bins, size_t n_bins, long long *__restrict__ chunk)
{
    __shared__ int part[4];
    const size_t base = (size_t)blockIdx.x * HIST_CHUNK;
    int c = 0;
#pragma unroll
    for (int u = 0; u < HIST_CHUNK / 256; u++) c += bin_used(bins, n_bins, base + u * 256 + threadIdx.x) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) chunk[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// the non-empty bins of a chunk, ascending, at the chunk's offset: thread t holds the bins base + 4t .. 4t + 3
__global__ __launch_bounds__(256) void hist_fill_kernel(const u64 *__restrict__ bins, size_t n_bins, const long long *__restrict__ chunk,
                                                        unsigned *__restrict__ value, u64 *__restrict__ within, u64 *__restrict__ between,
                                                        u64 *__restrict__ ungrouped)
{
    __shared__ int wave_sum[4];
    constexpr int PER = HIST_CHUNK / 256;
    const size_t base = (size_t)blockIdx.x * HIST_CHUNK + (size_t)threadIdx.x * PER;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    bool used[PER];
    int c = 0;
#pragma unroll
    for (int u = 0; u < PER; u++) { used[u] = bin_used(bins, n_bins, base + u); c += used[u] ? 1 : 0; }
    int incl = c;                                                  // inclusive scan across the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wave_sum[w] = incl;
    __syncthreads();
    long long o = chunk[blockIdx.x] + incl - c;
    for (int q = 0; q < w; q++) o += wave_sum[q];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        if (!used[u]) continue;
        const size_t b = base + u;
        value[o] = (unsigned)b;
        within[o] = bins[b];
        between[o] = bins[n_bins + b];
        ungrouped[o] = bins[2 * n_bins + b];
        o++;
    }
}

// workgroups per launch at most (TRACS_HIST_GRID: diagnostics, for measurements).  2 048: all of them resident at 8 per CU; the
// sweep is in DESIGN.md 3.11 and profiles/histogram/variant_*.json
unsigned hist_grid()
{
    const long c = tracs::sw::integer(tracs::sw::TRACS_HIST_GRID, 0L);
    return (c >= 1 && c <= 65535) ? (unsigned)c : 2048u;
}

}  // namespace

using namespace tracs;

extern "C" {

size_t tracs_hist_state_bytes(size_t n_bins) { return (n_bins < 1 || n_bins > 0x80000000ull) ? 0 : hist_bytes(n_bins); }

int tracs_hist_init(void *state, size_t n_bins, void *stream_)
{
    if (n_bins < 1 || n_bins > 0x80000000ull) { set_error("tracs_hist_init: n_bins must be in [1, 2^31]"); return TRACS_E_ARG; }
    if (!state) { set_error("tracs_hist_init: NULL state"); return TRACS_E_ARG; }
    TRACS_HIP_CHECK(hipMemsetAsync(state, 0, hist_bytes(n_bins), static_cast<hipStream_t>(stream_)));
    return TRACS_OK;
}

int tracs_hist_update(const uint32_t *dist, size_t ld, size_t n, size_t row_begin, size_t row_end, size_t col_begin,
                      int32_t dist_threshold, const int32_t *group, void *state, size_t n_bins, void *stream_)
{
    if (n_bins < 1 || n_bins > 0x80000000ull) { set_error("tracs_hist_update: n_bins must be in [1, 2^31]"); return TRACS_E_ARG; }
    if (!dist || !state) { set_error("tracs_hist_update: NULL argument"); return TRACS_E_ARG; }
    if (n >= (1ull << 30)) { set_error("tracs_hist_update: n must be below 2^30"); return TRACS_E_ARG; }
    if (ld < n) { set_error("tracs_hist_update: ld < n"); return TRACS_E_ARG; }
    if (row_end > n) row_end = n;
    if (row_end <= row_begin || dist_threshold < 0 || col_begin >= n) return TRACS_OK;     // no row, no column, or no cell within the threshold
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t nrows = row_end - row_begin;
    const unsigned grid = (unsigned)std::min<size_t>((nrows + 3) / 4, hist_grid());
    const unsigned flush_every = (unsigned)std::max<size_t>(1, 0xFFFFFFFFull / (4 * std::max<size_t>(n, 1)));
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream, dist, ld, (unsigned)n, (unsigned)row_begin, (unsigned)row_end,
                           (unsigned)col_begin, (unsigned)dist_threshold, group, static_cast<u64 *>(state), (unsigned)n_bins, flush_every);
    };
    if (group) launch(hist_panel_kernel<3>);
    else launch(hist_panel_kernel<1>);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

int tracs_hist_update_coo(const uint32_t *rows, const uint32_t *cols, const uint32_t *val, size_t m, const int32_t *group, void *state,
                          size_t n_bins, void *stream_)
{
    if (n_bins < 1 || n_bins > 0x80000000ull) { set_error("tracs_hist_update_coo: n_bins must be in [1, 2^31]"); return TRACS_E_ARG; }
    if (!state || (m && !val) || (m && group && !(rows && cols))) { set_error("tracs_hist_update_coo: NULL argument"); return TRACS_E_ARG; }
    if (!m) return TRACS_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const unsigned grid = (unsigned)std::min<size_t>((m + 255) / 256, hist_grid());
    if (group)
        hipLaunchKernelGGL(hist_coo_kernel<3>, dim3(grid), dim3(256), 0, stream, rows, cols, val, m, group, static_cast<u64 *>(state), (unsigned)n_bins);
    else
        hipLaunchKernelGGL(hist_coo_kernel<1>, dim3(grid), dim3(256), 0, stream, rows, cols, val, m, group, static_cast<u64 *>(state), (unsigned)n_bins);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

int tracs_hist_emit(void *state, size_t n_bins, size_t *n_rows, uint32_t *value, uint64_t *within, uint64_t *between, uint64_t *ungrouped,
                    void *stream_)
{
    if (n_rows) *n_rows = 0;
    if (n_bins < 1 || n_bins > 0x80000000ull) { set_error("tracs_hist_emit: n_bins must be in [1, 2^31]"); return TRACS_E_ARG; }
    if (!state || !n_rows) { set_error("tracs_hist_emit: NULL argument"); return TRACS_E_ARG; }
    const bool fill = value || within || between || ungrouped;
    if (fill && !(value && within && between && ungrouped)) {
        set_error("tracs_hist_emit: value, within, between and ungrouped are all given or all NULL");
        return TRACS_E_ARG;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const u64 *bins = hist_bins(state);
    long long *chunk = hist_chunk_words(state, n_bins);
    const size_t nc = hist_chunks(n_bins);
    hipLaunchKernelGGL(hist_count_kernel, dim3((unsigned)nc), dim3(256), 0, stream, bins, n_bins, chunk);
    hipLaunchKernelGGL(scan_i64_inplace_kernel, dim3(1), dim3(1024), 0, stream, chunk, nc);
    TRACS_HIP_CHECK(hipGetLastError());
    u64 over = 0;
    long long total = 0;
    TRACS_HIP_CHECK(hipMemcpyAsync(&over, state, 8, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipMemcpyAsync(&total, chunk + nc, 8, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    if (over) {
        set_error("tracs_hist_emit: " + std::to_string(over) + " values were offered that are not below n_bins = " + std::to_string(n_bins) +
                  "; the histogram is incomplete");
        return TRACS_E_ARG;
    }
    *n_rows = (size_t)total;
    if (fill && total) {
        hipLaunchKernelGGL(hist_fill_kernel, dim3((unsigned)nc), dim3(256), 0, stream, bins, n_bins, chunk, value,
                           reinterpret_cast<u64 *>(within), reinterpret_cast<u64 *>(between), reinterpret_cast<u64 *>(ungrouped));
        TRACS_HIP_CHECK(hipGetLastError());
        TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    }
    return TRACS_OK;
}

// tests only: out[0..2] = the cells the state's updates counted by route (combined, lds, global), out[3] = the LDS slots per class
int tracs_debug_hist_routes(const void *state, double *out)
{
    if (!state || !out) return 0;
    u64 h[HIST_HEADER];
    TRACS_HIP_CHECK(hipDeviceSynchronize());
    TRACS_HIP_CHECK(hipMemcpy(h, state, sizeof h, hipMemcpyDeviceToHost));
    out[0] = (double)h[1]; out[1] = (double)h[2]; out[2] = (double)h[3]; out[3] = (double)HIST_W;
    return 4;
}

}  // extern "C"
