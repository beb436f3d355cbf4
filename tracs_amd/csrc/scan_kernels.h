// scan_kernels.h -- the exclusive scans shared between files.  Included by .hip files only.
//   offsets_scan_launch       per-pair counts (uint32) into list offsets, three launches (filter.hip: a pair's SNP positions;
//                             pair_sites.hip: its SNP entries)
//   scan_i64_inplace_kernel   int64 counts into offsets in place, one workgroup (pairsnp.hip: rows of the COO output; nearest.hip:
//                             the samples' lists; histogram.hip: the chunks' non-empty bins)
#pragma once
#include "common.h"

#include <algorithm>

namespace tracs {

// off[0 .. n] on the device: exclusive scan of d[0 .. n) in three launches (tiles of 1 024)
static __global__ __launch_bounds__(256) void offsets_tile_sums_kernel(const unsigned *__restrict__ d, size_t n, unsigned long long *__restrict__ sums)
{
    __shared__ unsigned long long part[4];
    const size_t base = (size_t)blockIdx.x * 1024;
    unsigned long long s = 0;
    for (int k = 0; k < 4; k++) { const size_t t = base + (size_t)k * 256 + threadIdx.x; if (t < n) s += d[t]; }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
static __global__ __launch_bounds__(1024) void offsets_scan_sums_kernel(unsigned long long *__restrict__ sums, size_t tiles)
{
    __shared__ unsigned long long part[1024];
    const size_t per = (tiles + 1023) / 1024, b = std::min(tiles, (size_t)threadIdx.x * per), e = std::min(tiles, b + per);
    unsigned long long s = 0;
    for (size_t k = b; k < e; k++) s += sums[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (unsigned st = 1; st < 1024; st <<= 1) {
        const unsigned long long v = threadIdx.x >= st ? part[threadIdx.x - st] : 0ull;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = part[threadIdx.x] - s;
    for (size_t k = b; k < e; k++) { const unsigned long long v = sums[k]; sums[k] = run; run += v; }
}
static __global__ __launch_bounds__(256) void offsets_fill_kernel(const unsigned *__restrict__ d, size_t n, const unsigned long long *__restrict__ sums,
                                                             long long *__restrict__ off)
{
    __shared__ unsigned long long wsum[4];
    const size_t base = (size_t)blockIdx.x * 1024 + (size_t)threadIdx.x * 4;
    unsigned v[4];
    unsigned long long s = 0;
    for (int k = 0; k < 4; k++) { v[k] = base + k < n ? d[base + k] : 0u; s += v[k]; }
    unsigned long long incl = s;
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long x = __shfl_up(incl, o, 64); if (lane >= o) incl += x; }
    if (lane == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    unsigned long long run = sums[blockIdx.x] + incl - s;
    for (unsigned w = 0; w < (threadIdx.x >> 6); w++) run += wsum[w];
    // (n + 1 offsets: index n takes the total)
    for (int k = 0; k < 4; k++) { if (base + k <= n) off[base + k] = (long long)run; run += v[k]; }
}

// off[0 .. n] <- the exclusive scan of d[0 .. n) (off[n]: the total).  sums: device scratch of offsets_scan_sums(n) words.
static inline size_t offsets_scan_sums(size_t n) { return n / 1024 + 2; }
static int offsets_scan_launch(const unsigned *d, size_t n, unsigned long long *sums, long long *off, hipStream_t stream)
{
    const size_t tiles = (n + 1023) / 1024;
    // (n + 1 offsets: the tile that holds index n writes off[n]; when n is a multiple of 1 024 that is one tile more)
    const size_t otiles = n / 1024 + 1;
    TRACS_HIP_CHECK(hipMemsetAsync(sums, 0, (otiles + 1) * 8, stream));
    if (tiles) hipLaunchKernelGGL(offsets_tile_sums_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, d, n, sums);
    hipLaunchKernelGGL(offsets_scan_sums_kernel, dim3(1), dim3(1024), 0, stream, sums, otiles);
    hipLaunchKernelGGL(offsets_fill_kernel, dim3((unsigned)otiles), dim3(256), 0, stream, d, n, sums, off);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

// In place: counts[0 .. n) -> exclusive offsets counts[0 .. n] (index n takes the total).  One workgroup of 1 024, serial over tiles of
// 1 024 (n up to a few 100k).
static __global__ __launch_bounds__(1024) void scan_i64_inplace_kernel(long long *__restrict__ counts, size_t n)
{
    __shared__ long long part[1024];
    __shared__ long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (size_t base = 0; base < n + 1; base += 1024) {
        const size_t idx = base + threadIdx.x;
        const long long v = idx < n ? counts[idx] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const long long t = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += t;
            __syncthreads();
        }
        const long long incl = part[threadIdx.x];
        const long long c0 = carry;
        __syncthreads();
        if (idx <= n) counts[idx] = c0 + incl - v;
        if (threadIdx.x == 1023) carry = c0 + incl;
        __syncthreads();
    }
}

}  // namespace tracs
