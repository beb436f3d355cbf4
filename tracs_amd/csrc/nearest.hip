// nearest.hip -- per-sample k nearest neighbours over the dense pair panels (tracs_knn_*, include/tracs_hip.h).
//
// A candidate j of sample s is ranked by the 64-bit key (d(s, j) << 32) | j: SNP distance first, then the sample index.  The index
// makes every key of a list unique, so the order is total and the lists do not depend on panel splits or launch order.
//
// State: one block per list, knn_stride(K) bytes: K keys (uint64, ascending, KNN_SENT beyond the last neighbour found) followed by
// their K compared-site counts (uint32).  An update merges one row panel of dist / ncomp (indexed by ABSOLUTE row, leading
// dimension ld, the cells tracs_pairsnp_dense writes: j >= max(col_begin, i + 1)) into the lists in two stream-ordered launches:
//   row part     knn_row_kernel: one wave per panel row i offers (d(i, j), j) to list i;
//   column part  knn_col_kernel (one-file mode): one workgroup per strip of 32 columns offers (d(i, c), i) to list c for the
//                panel's rows i < c.
// Each launch owns disjoint lists, so no list has two writers.  Both read the panel coalesced, each cell once: a wave of the row
// part reads 64 consecutive cells of its row, a wave of the column part two 128-byte row segments of its strip.
//
// Selection (block select): a list's current K-th key is the bar; a cell whose key is below the bar is staged in LDS.  A stage of
// up to 64 keys is sorted across one wave (bitonic network over __shfl_xor) and merged into the list by rank: a list entry moves
// down by the number of staged keys below it (binary search over the stage with __shfl), a staged key lands at its stage position
// plus the number of list keys below it (binary search over the list).  What lands at K or beyond is dropped.  The compared-site
// count of a staged cell is read from ncomp when it is merged, while the panel is resident.
#include "common.h"
#include "pair_select.h"     // grid_for
#include "scan_kernels.h"

#include <algorithm>

namespace {

constexpr unsigned long long KNN_SENT = ~0ull;
constexpr int KNN_KMAX = 1024;
constexpr int KNN_CW = 32;          // columns per workgroup of the column part (one 128-byte line of a row)
constexpr size_t KNN_MAX_BLOCKS = 65536;     // of the grid-stride kernels (init, fill)

inline size_t knn_stride(int k) { return ((size_t)k * 12 + 15) / 16 * 16; }

__device__ __forceinline__ unsigned long long *list_keys(void *state, size_t l, size_t stride)
{
    return reinterpret_cast<unsigned long long *>(static_cast<char *>(state) + l * stride);
}

__device__ __forceinline__ unsigned long long umin64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a < b ? b : a; }

// ascending bitonic sort of one key per lane across the wave
__device__ __forceinline__ unsigned long long wave_sort64(unsigned long long v, int lane)
{
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const unsigned long long o = __shfl_xor(v, j, 64);
            v = (((lane & j) == 0) == ((lane & k) == 0)) ? umin64(v, o) : umax64(v, o);
        }
    return v;
}

// Merge a sorted stage (s: one key per lane, KNN_SENT in unused lanes; snn: its compared-site count) into the list (lk, ln) of K
// <= 64 * KT entries.  All 64 lanes call it.  Returns the list's new K-th key (uniform).
template <int KT>
__device__ unsigned long long wave_merge(unsigned long long *__restrict__ lk, unsigned *__restrict__ ln, int K, unsigned long long s,
                                         unsigned snn, int lane)
{
    unsigned long long key[KT];
    unsigned nn[KT];
    int dst[KT];
#pragma unroll
    for (int t = 0; t < KT; t++) {
        const int p = lane + 64 * t;
        key[t] = p < K ? lk[p] : KNN_SENT;
        nn[t] = p < K ? ln[p] : 0u;
    }
    // the staged key's rank in the list
    int r = 0;
    if (s != KNN_SENT)
        for (int b = 64 * KT; b; b >>= 1)
            if (r + b <= K && lk[r + b - 1] < s) r += b;
    // each list key's rank in the stage
#pragma unroll
    for (int t = 0; t < KT; t++) {
        int c = 0;
#pragma unroll
        for (int b = 64; b; b >>= 1) {
            const unsigned long long sv = __shfl(s, min(c + b - 1, 63), 64);
            if (c + b <= 64 && sv < key[t]) c += b;
        }
        dst[t] = lane + 64 * t + c;
    }
    // every read of the list above has been consumed: the writes below cannot overtake one
    __builtin_amdgcn_wave_barrier();
    unsigned long long kth = KNN_SENT;
#pragma unroll
    for (int t = 0; t < KT; t++)
        if (key[t] != KNN_SENT && dst[t] < K) {
            lk[dst[t]] = key[t];
            ln[dst[t]] = nn[t];
            if (dst[t] == K - 1) kth = key[t];
        }
    if (s != KNN_SENT && lane + r < K) {
        lk[lane + r] = s;
        ln[lane + r] = snn;
        if (lane + r == K - 1) kth = s;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kth = umin64(kth, __shfl_xor(kth, o, 64));
    return kth;
}

// Insert m unsorted staged keys into a list of K <= 64 entries held one per lane (lk, ln in LDS), key by key: a key below the K-th
// moves the lanes above its rank up by one (__shfl_up).  A stage of a few keys costs a few ballots instead of a 64-wide sort and
// merge.  nn of an inserted key is 0 (the column part reads it after its walk).  All 64 lanes call it.  Returns the new K-th key.
__device__ unsigned long long wave_insert(unsigned long long *lk, unsigned *ln, int K, const unsigned long long *stage, int m, int lane)
{
    unsigned long long key = lane < K ? lk[lane] : KNN_SENT;
    unsigned nn = lane < K ? ln[lane] : 0u;
    unsigned long long kth = __shfl(key, K - 1, 64);
    for (int q = 0; q < m; q++) {
        const unsigned long long x = stage[q];
        if (x >= kth) continue;                                   // uniform
        const int pos = __popcll(__ballot(key < x));
        const unsigned long long up = __shfl_up(key, 1, 64);
        const unsigned upn = __shfl_up(nn, 1, 64);
        if (lane > pos) { key = up; nn = upn; }
        else if (lane == pos) { key = x; nn = 0u; }
        kth = __shfl(key, K - 1, 64);
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < K) { lk[lane] = key; ln[lane] = nn; }
    return kth;
}

// Row part: wave w of the workgroup takes panel row i = row_begin + 4 * blockIdx.x + w.
template <int KT>
__global__ __launch_bounds__(256) void knn_row_kernel(const unsigned *__restrict__ dist, const unsigned *__restrict__ ncomp, size_t ld,
                                                      unsigned n, unsigned row_begin, unsigned row_end, unsigned col_begin, unsigned thr,
                                                      int K, size_t stride, void *state)
{
    __shared__ unsigned long long stage[4][64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned i = row_begin + blockIdx.x * 4 + w;
    if (i >= row_end) return;                                   // per wave: nothing below synchronises the workgroup
    unsigned long long *lk = list_keys(state, i, stride);
    unsigned *ln = reinterpret_cast<unsigned *>(lk + K);
    unsigned long long bar = lk[K - 1];
    const unsigned *row = dist + (size_t)i * ld;
    const unsigned *nrow = ncomp + (size_t)i * ld;
    const unsigned long long below = (1ull << lane) - 1ull;
    int cnt = 0;
    auto flush = [&]() {
        unsigned long long s = lane < cnt ? stage[w][lane] : KNN_SENT;
        s = wave_sort64(s, lane);
        const unsigned snn = s != KNN_SENT ? nrow[(unsigned)s] : 0u;
        bar = wave_merge<KT>(lk, ln, K, s, snn, lane);
        cnt = 0;
    };
    for (unsigned j0 = max(col_begin, i + 1); j0 < n; j0 += 256) {
        unsigned v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const unsigned j = j0 + 64 * u + lane;
            v[u] = j < n ? row[j] : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const unsigned j = j0 + 64 * u + lane;
            const unsigned long long key = (j < n && v[u] <= thr) ? ((unsigned long long)v[u] << 32 | j) : KNN_SENT;
            unsigned long long m = __ballot(key < bar);
            if (!m) continue;
            if (cnt + __popcll(m) > 64) {
                flush();
                m = __ballot(key < bar);
            }
            if (key < bar) stage[w][cnt + __popcll(m & below)] = key;
            cnt += __popcll(m);
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (cnt) flush();
}

// Column part: the workgroup owns columns [c0, c0 + 32) and walks the panel's rows i < c in tiles of 64 rows (thread: column
// threadIdx.x % 32, rows threadIdx.x / 32 + 8u; the next tile's cells are loaded before the current one is staged).  A tile stages
// at most 64 keys per column; then the four waves merge the columns that staged any, eight columns each.  With K <= 64 the strip's
// lists live in LDS for the whole walk (a column far down the matrix takes a merge in most tiles: ~K ln(c / K) keys pass its bar)
// and go back to the state at the end, and a stage goes in key by key (wave_insert: a column far down takes a few keys in most tiles,
// where a 64-wide sort and merge per tile made the walk merge-bound); larger K merge into the state in place.  The compared-site counts of the kept keys are read
// after the walk, in one round: a read per merge put a global load's latency into every tile that merged.
template <int KT>
__global__ __launch_bounds__(256) void knn_col_kernel(const unsigned *__restrict__ dist, const unsigned *__restrict__ ncomp, size_t ld,
                                                      unsigned n, unsigned row_begin, unsigned row_end, unsigned col_lo, unsigned thr,
                                                      int K, size_t stride, void *state)
{
    constexpr bool LDS_LISTS = KT == 1;
    __shared__ unsigned long long stage[KNN_CW][64];
    __shared__ unsigned long long bar[KNN_CW];
    __shared__ int cnt[KNN_CW];
    __shared__ unsigned long long lds_keys[LDS_LISTS ? KNN_CW : 1][64];
    __shared__ unsigned lds_nn[LDS_LISTS ? KNN_CW : 1][64];
    const unsigned c0 = col_lo + blockIdx.x * KNN_CW;
    const int tc = threadIdx.x & (KNN_CW - 1), tr = threadIdx.x / KNN_CW;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned c = c0 + tc;
    const unsigned ncol = min((unsigned)KNN_CW, n - c0);
    if (LDS_LISTS)
        for (int t = threadIdx.x; t < KNN_CW * 64; t += 256) {
            const int q = t / 64, e = t % 64;
            const unsigned long long *g = list_keys(state, c0 + q, stride);
            const bool in = q < (int)ncol && e < K;
            lds_keys[q][e] = in ? g[e] : KNN_SENT;
            lds_nn[q][e] = in ? reinterpret_cast<const unsigned *>(g + K)[e] : 0u;
        }
    __syncthreads();
    if (threadIdx.x < KNN_CW) {
        bar[tc] = c < n ? (LDS_LISTS ? lds_keys[tc][K - 1] : list_keys(state, c, stride)[K - 1]) : 0ull;     // a column past n takes nothing
        cnt[tc] = 0;
    }
    __syncthreads();
    const unsigned i_stop = min(row_end, c0 + ncol - 1);                      // rows below the strip's last column
    unsigned v[8];
    auto load = [&](unsigned i0, unsigned *dst) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const unsigned i = i0 + tr + 8 * u;
            dst[u] = (i < i_stop && i < c && c < n) ? dist[(size_t)i * ld + c] : 0xFFFFFFFFu;
        }
    };
    if (row_begin < i_stop) load(row_begin, v);
    for (unsigned i0 = row_begin; i0 < i_stop; i0 += 64) {
        unsigned nv[8];
        load(i0 + 64, nv);
        const unsigned long long b = bar[tc];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const unsigned i = i0 + tr + 8 * u;
            const unsigned long long key = v[u] <= thr ? ((unsigned long long)v[u] << 32 | i) : KNN_SENT;
            if (key < b) stage[tc][atomicAdd(&cnt[tc], 1)] = key;
        }
        __syncthreads();
        for (int q = w; q < KNN_CW; q += 4) {
            const int m = cnt[q];
            if (!m) continue;
            unsigned long long nb;                                   // nn: read once the walk is done
            if (LDS_LISTS) {
                nb = wave_insert(lds_keys[q], lds_nn[q], K, stage[q], m, lane);
            } else {
                unsigned long long s = lane < m ? stage[q][lane] : KNN_SENT;
                s = wave_sort64(s, lane);
                unsigned long long *lk = list_keys(state, c0 + q, stride);
                nb = wave_merge<KT>(lk, reinterpret_cast<unsigned *>(lk + K), K, s, 0u, lane);
            }
            if (lane == 0) { bar[q] = nb; cnt[q] = 0; }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = nv[u];
    }
    // the compared-site counts of the keys this walk kept (row index i < c inside the panel), all in one round of loads; the others
    // keep theirs.  With LDS lists the lists go back to the state.
    for (int t = threadIdx.x; t < (int)ncol * K; t += 256) {
        const int q = t / K, e = t % K;
        const unsigned cq = c0 + q;
        unsigned long long *g = list_keys(state, cq, stride);
        unsigned *gn = reinterpret_cast<unsigned *>(g + K);
        const unsigned long long key = LDS_LISTS ? lds_keys[q][e] : g[e];
        const unsigned i = (unsigned)key;
        const bool here = key != KNN_SENT && i < cq && i >= row_begin && i < row_end;
        if (LDS_LISTS) {
            g[e] = key;
            gn[e] = here ? ncomp[(size_t)i * ld + cq] : lds_nn[q][e];
        } else if (here) {
            gn[e] = ncomp[(size_t)i * ld + cq];
        }
    }
}

__global__ __launch_bounds__(256) void knn_init_kernel(void *state, size_t n_lists, int K, size_t stride)
{
    const size_t total = n_lists * (size_t)K;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        unsigned long long *lk = list_keys(state, t / K, stride);
        const int e = (int)(t % K);
        lk[e] = KNN_SENT;
        reinterpret_cast<unsigned *>(lk + K)[e] = 0u;
    }
}

// neighbours found per list (the keys below KNN_SENT are a prefix)
__global__ __launch_bounds__(256) void knn_count_kernel(void *state, size_t list_begin, size_t nl, int K, size_t stride,
                                                        long long *__restrict__ counts)
{
    const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= nl) return;
    const unsigned long long *lk = list_keys(state, list_begin + l, stride);
    int r = 0;
    for (int b = KNN_KMAX; b; b >>= 1)
        if (r + b <= K && lk[r + b - 1] != KNN_SENT) r += b;
    counts[l] = r;
}

__global__ __launch_bounds__(256) void knn_fill_kernel(void *state, size_t list_begin, size_t nl, int K, size_t stride,
                                                       const long long *__restrict__ offsets, unsigned *__restrict__ rows,
                                                       unsigned *__restrict__ cols, unsigned *__restrict__ d, unsigned *__restrict__ nn)
{
    const size_t total = nl * (size_t)K;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t l = t / K;
        const int e = (int)(t % K);
        const unsigned long long *lk = list_keys(state, list_begin + l, stride);
        const unsigned long long key = lk[e];
        if (key == KNN_SENT) continue;
        const size_t o = (size_t)offsets[l] + e;
        rows[o] = (unsigned)(list_begin + l);
        cols[o] = (unsigned)key;
        d[o] = (unsigned)(key >> 32);
        nn[o] = reinterpret_cast<const unsigned *>(lk + K)[e];
    }
}

}  // namespace

using namespace tracs;

extern "C" {

size_t tracs_knn_state_bytes(size_t n_lists, int k)
{
    return (k < 1 || k > KNN_KMAX) ? 0 : n_lists * knn_stride(k);
}

int tracs_knn_init(void *state, size_t n_lists, int k, void *stream_)
{
    if (k < 1 || k > KNN_KMAX) { set_error("tracs_knn_init: k must be in [1, 1024]"); return TRACS_E_ARG; }
    if (!state && n_lists) { set_error("tracs_knn_init: NULL state"); return TRACS_E_ARG; }
    if (!n_lists) return TRACS_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(knn_init_kernel, dim3(grid_for(n_lists * (size_t)k, KNN_MAX_BLOCKS)), dim3(256), 0, stream, state, n_lists, k, knn_stride(k));
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

int tracs_knn_update(const uint32_t *dist, const uint32_t *ncomp, size_t ld, size_t n, size_t row_begin, size_t row_end,
                     size_t col_begin, int32_t dist_threshold, int k, int symmetric, void *state, void *stream_)
{
    if (k < 1 || k > KNN_KMAX) { set_error("tracs_knn_update: k must be in [1, 1024]"); return TRACS_E_ARG; }
    if (!dist || !ncomp || !state) { set_error("tracs_knn_update: NULL argument"); return TRACS_E_ARG; }
    if (n >= 0xFFFFFFFFull) { set_error("tracs_knn_update: n must be below 2^32 - 1"); return TRACS_E_ARG; }
    if (ld < n) { set_error("tracs_knn_update: ld < n"); return TRACS_E_ARG; }
    if (row_end > n) row_end = n;
    if (row_end <= row_begin || dist_threshold < 0) return TRACS_OK;     // no row, or no cell within the threshold
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t stride = knn_stride(k), nrows = row_end - row_begin;
    const unsigned thr = (unsigned)dist_threshold;
    auto launch = [&](auto row_kernel, auto col_kernel) {
        hipLaunchKernelGGL(row_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, stream, dist, ncomp, ld, (unsigned)n,
                           (unsigned)row_begin, (unsigned)row_end, (unsigned)col_begin, thr, k, stride, state);
        const size_t col_lo = std::max(col_begin, row_begin + 1);
        if (symmetric && col_lo < n)
            hipLaunchKernelGGL(col_kernel, dim3((unsigned)((n - col_lo + KNN_CW - 1) / KNN_CW)), dim3(256), 0, stream, dist, ncomp, ld,
                               (unsigned)n, (unsigned)row_begin, (unsigned)row_end, (unsigned)col_lo, thr, k, stride, state);
    };
    if (k <= 64) launch(knn_row_kernel<1>, knn_col_kernel<1>);
    else if (k <= 256) launch(knn_row_kernel<4>, knn_col_kernel<4>);
    else launch(knn_row_kernel<16>, knn_col_kernel<16>);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

int tracs_knn_emit(void *state, size_t list_begin, size_t list_end, int k, int64_t *offsets, uint32_t *rows, uint32_t *cols,
                   uint32_t *d, uint32_t *nn, void *stream_)
{
    if (k < 1 || k > KNN_KMAX) { set_error("tracs_knn_emit: k must be in [1, 1024]"); return TRACS_E_ARG; }
    if (!state || !offsets) { set_error("tracs_knn_emit: NULL argument"); return TRACS_E_ARG; }
    const bool fill = rows || cols || d || nn;
    if (fill && !(rows && cols && d && nn)) { set_error("tracs_knn_emit: rows, cols, d and nn are all given or all NULL"); return TRACS_E_ARG; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t nl = list_end > list_begin ? list_end - list_begin : 0;
    const size_t stride = knn_stride(k);
    long long *off = reinterpret_cast<long long *>(offsets);
    if (nl) hipLaunchKernelGGL(knn_count_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, stream, state, list_begin, nl, k, stride, off);
    hipLaunchKernelGGL(scan_i64_inplace_kernel, dim3(1), dim3(1024), 0, stream, off, nl);
    if (fill && nl)
        hipLaunchKernelGGL(knn_fill_kernel, dim3(grid_for(nl * (size_t)k, KNN_MAX_BLOCKS)), dim3(256), 0, stream, state, list_begin, nl, k, stride, off,
                           rows, cols, d, nn);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

}  // extern "C"
