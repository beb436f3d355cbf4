// pair_select.h -- what the states that select pairs share (forest.hip, ancestors.hip; the union-find also cluster.hip, grid_for also
// nearest.hip): ordered 64-bit keys, the segmented wave minimum, the union-find, the state arena, the header read-back, the sort by
// i << 32 | j and the value columns kept with a pair.  Free functions and two small structs.  Included by .hip files only.
#pragma once
#include "common.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

namespace tracs {

// ---- ordered 64-bit keys ---------------------------------------------------------------------------------------------------------
constexpr unsigned long long KEY_NONE = ~0ull;                     // no candidate: above every key
constexpr unsigned long long KEY_NAN = 0xFFF8000000000000ull;      // every NaN: above every number's key (either direction), below KEY_NONE
constexpr unsigned NO_VERTEX = 0xFFFFFFFFu;                        // no component / target / parent / winner

// ascending: numbers in order (the sign flip), -0.0 == +0.0, +inf at 0xFFF0..., every NaN at KEY_NAN
__device__ __forceinline__ unsigned long long f64_key_up(double x)
{
    if (x != x) return KEY_NAN;
    if (x == 0.0) return 0x8000000000000000ull;
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// descending: the largest number first, -0.0 == +0.0, -inf (0xFFF0...) last of the numbers, every NaN after it
__device__ __forceinline__ unsigned long long f64_key_down(double x)
{
    if (x != x) return KEY_NAN;
    return ~f64_key_up(x);
}

// ---- wave reductions in front of an atomic ---------------------------------------------------------------------------------------
// minimum of v over the lanes at and above this one that hold the same target c (runs of one c are what row-major COO gives); lanes
// of other runs of the same c may contribute too, which is harmless.  All 64 lanes call it.
__device__ __forceinline__ unsigned long long seg_min(unsigned long long v, unsigned c, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long ov = __shfl_down(v, off, 64);
        const unsigned oc = __shfl_down(c, off, 64);
        if (lane + off < 64 && oc == c && ov < v) v = ov;
    }
    return v;
}

// one atomicMin per run of equal targets in the wave, and only when it can lower the value: dst[] only decreases while a pass runs,
// so a plain (possibly stale) read is an upper bound of the current value, and a candidate at or above it cannot win.  That test
// also keeps KEY_NONE out: dst[c] <= KEY_NONE always.  c == NO_VERTEX: the lane has no target.
__device__ __forceinline__ void wave_min_into(unsigned long long *dst, unsigned long long v, unsigned c, int lane)
{
    const unsigned long long m = seg_min(v, c, lane);
    const unsigned prev = __shfl_up(c, 1, 64);
    if (c != NO_VERTEX && (lane == 0 || prev != c) && m < dst[c]) atomicMin(&dst[c], m);
}

// the wave's sum of cnt -> *dst: one atomicAdd per wave, none for a sum of 0.  All 64 lanes call it.
__device__ __forceinline__ void wave_add_into(unsigned long long *dst, unsigned long long cnt, int lane)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (lane == 0 && cnt) atomicAdd(dst, cnt);
}

// ---- lock-free union-find --------------------------------------------------------------------------------------------------------
// parent[] only ever moves a node towards smaller ids (hook larger root under smaller, path halving), so a stale read still lands on
// a valid ancestor: races cost retries, never a wrong component.  Agent-scope relaxed atomics keep the loads out of the
// (non-coherent) vector L1.
__device__ __forceinline__ int uf_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(int *parent, int x)
{
    for (;;) {
        const int p = uf_load(&parent[x]);
        if (p == x) return x;
        const int gp = uf_load(&parent[p]);
        if (gp != p) __hip_atomic_store(&parent[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // path halving
        x = gp;
    }
}

// ---- the values kept with a pair: the columns its CSV row is written with ----------------------------------------------------------
// As a batch's input a column may be NULL (the value is 0), as emit's output too (the column is not wanted); a state's are all there.
struct PairColumns { unsigned *d, *nn, *f; double *p, *e; };

// a batch's columns are only read
static inline PairColumns batch_columns(const uint32_t *d, const uint32_t *nn, const uint32_t *f, const double *p, const double *e)
{
    return PairColumns{const_cast<unsigned *>(d), const_cast<unsigned *>(nn), const_cast<unsigned *>(f), const_cast<double *>(p), const_cast<double *>(e)};
}

// dst[k] <- src[q]; a NULL column of src gives 0
__device__ __forceinline__ void take_columns(const PairColumns &dst, size_t k, const PairColumns &src, size_t q)
{
    dst.d[k] = src.d ? src.d[q] : 0u; dst.nn[k] = src.nn ? src.nn[q] : 0u; dst.f[k] = src.f ? src.f[q] : 0u;
    dst.p[k] = src.p ? src.p[q] : 0.0; dst.e[k] = src.e ? src.e[q] : 0.0;
}

// dst[k] <- src[q], every column there
__device__ __forceinline__ void copy_columns(const PairColumns &dst, size_t k, const PairColumns &src, size_t q)
{
    dst.d[k] = src.d[q]; dst.nn[k] = src.nn[q]; dst.f[k] = src.f[q]; dst.p[k] = src.p[q]; dst.e[k] = src.e[q];
}

// out[k] <- src[q]; a NULL column of out is skipped
__device__ __forceinline__ void emit_columns(const PairColumns &out, size_t k, const PairColumns &src, size_t q)
{
    if (out.d) out.d[k] = src.d[q];
    if (out.nn) out.nn[k] = src.nn[q];
    if (out.f) out.f[k] = src.f[q];
    if (out.p) out.p[k] = src.p[q];
    if (out.e) out.e[k] = src.e[q];
}

// ---- state arena -----------------------------------------------------------------------------------------------------------------
// A cursor that hands out typed arrays, each 256-byte aligned, from a base address.  A struct lists its arrays once, in a constructor
// S(base, n, &bytes); the same walk over base 0 only measures (arena_bytes), so a size and a layout cannot drift apart.
struct Arena {
    uintptr_t base;
    size_t used = 0, *total;                                       // *total (when given) follows `used`
    Arena(void *b, size_t *total_) : base(reinterpret_cast<uintptr_t>(b)), total(total_) {}
    template <class T>
    T *take(size_t count)
    {
        const size_t at = used;
        used += (count * sizeof(T) + 255) / 256 * 256;
        if (total) *total = used;
        return reinterpret_cast<T *>(base + at);
    }
};

template <class S>
size_t arena_bytes(size_t n) { size_t bytes = 0; (void)S(nullptr, n, &bytes); return bytes; }

// h <- the state's header; `who` fails when the state was initialised for another vertex count than n (Hdr has a member n)
template <class Hdr>
int read_state_header(const Hdr *hdr_dev, size_t n, const char *who, hipStream_t stream, Hdr *h)
{
    TRACS_HIP_CHECK(hipMemcpyAsync(h, hdr_dev, sizeof(Hdr), hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    if (h->n != n) { set_error(std::string(who) + ": the state was initialised for another vertex count"); return TRACS_E_ARG; }
    return TRACS_OK;
}

// ---- emit ------------------------------------------------------------------------------------------------------------------------
// keys[0 .. count) = i << 32 | j with idx[0 .. count) beside them, both buffers 2 x capacity long: sorted by key (rocprim radix sort)
// into keys + capacity, idx + capacity.  slot: the sort's temporary storage.
static int sort_by_pair_key(unsigned long long *keys, unsigned *idx, size_t count, size_t capacity, WsSlot slot, hipStream_t stream)
{
    size_t tmp_bytes = 0;
    TRACS_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, keys + capacity, idx, idx + capacity, count, 0u, 64u, stream));
    char *tmp;
    int rc;
    if ((rc = workspace_get(slot, std::max<size_t>(tmp_bytes, 1), &tmp))) return rc;
    TRACS_HIP_CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, keys + capacity, idx, idx + capacity, count, 0u, 64u, stream));
    return TRACS_OK;
}

// blocks of 256 threads for a grid-stride loop over `work` items: at least one, at most cap (SELECT_BLOCKS: the selection states')
constexpr size_t SELECT_BLOCKS = 4096;
inline unsigned grid_for(size_t work, size_t cap) { return (unsigned)std::max<size_t>(1, std::min<size_t>((work + 255) / 256, cap)); }

}  // namespace tracs
