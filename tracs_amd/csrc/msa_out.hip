// msa_out.hip -- planes back to text, and what is in every column.
//
// Every rule of `tracs distance` is defined through the alignment it leaves (3.12, 3.13); that alignment exists only as packed planes.
// This file is the way back and the view into it:
//
//     site_census_kernel   per site: the samples whose allele mask is exactly A, C, G, T, N (all four), or a partial code, and whether
//                          the site DIFFERS -- two samples with disjoint masks, the condition under which it adds 1 to some d(i, j)
//     unpack_kernel        samples [first, first + count) -> canonical text ("XACMGRSVTWYHKDBN"[mask]), one row per sample
#include "common.h"
#include "debug_api.h"

#include <algorithm>
#include <cstring>
#include <string>

namespace tracs {

// ---------------------------------------------------------------------------------------------------------------------------------
// The differs table, from the definition: bit p of the table, p = the 14-bit presence word of a site (bit m - 1: some sample has the
// mask m, m = 1 .. 14; N = 15 is disjoint from nothing and takes no part), is set iff two present masks have an empty intersection.
constexpr int DIFFERS_WORDS = (1 << 14) / 32;
static const unsigned *differs_table()
{
    static unsigned table[DIFFERS_WORDS];
    static const bool built = [] {
        for (unsigned p = 0; p < (1u << 14); p++) {
            bool d = false;
            for (unsigned a = 1; a <= 14 && !d; a++)
                for (unsigned b = a + 1; b <= 14 && !d; b++)
                    d = ((p >> (a - 1)) & 1u) && ((p >> (b - 1)) & 1u) && (a & b) == 0u;
            if (d) table[p >> 5] |= 1u << (p & 31u);
        }
        return true;
    }();
    (void)built;
    return table;
}

__device__ unsigned g_differs_table[DIFFERS_WORDS];

// ---------------------------------------------------------------------------------------------------------------------------------
// Census.  ONE kernel for the counts and the differs bitmap: both are functions of the same four allele planes, and a second kernel
// would read them a second time (the stored N plane is A & C & G & T by construction, so four planes are read, not five).
// One workgroup = one group of 128 sites.  A thread is one (sample lane, 32-site word): thread t reads word t & 3 of sample lane
// t >> 2, so a wave's load of one (group, plane) run is 16 samples x 16 bytes = 256 contiguous bytes, four bytes per lane.  (With a
// whole uint4 per lane, site_n_count_kernel's form, the five counters and the presence words are 4 x as many registers: 256 VGPRs,
// one wave per SIMD.  This form needs 1 / 4 of those and runs four.)  A lane turns its word of the four planes into the minterms it
// needs: the four one-hot masks and N feed bit-sliced counters (CS_PLANES one-bit columns, a ripple-carry add per loaded word), the
// ten partial codes are OR-ed into presence words; `other` is n minus the five counts (inside a packed sample no mask is 0).  The
// counters are flushed through LDS once per CS_CHUNK samples per lane, one category at a time, stored word-major so that thread t
// sums bit (t & 31) of word (t >> 5) & 3 over the 32 sample lanes of its half of the workgroup with eight 16-byte reads per plane.
// Presence is OR-reduced over the lanes of one word by shuffles, over the waves in LDS.  The thread that owns a site then has its five
// totals -- a one-hot mask is present iff its count is not 0 -- and the ten presence bits: the 14-bit presence word indexes the
// differs table.  Pad samples (s >= n) are never loaded.  Reads n x groups x 64 bytes, writes 6 x 4 bytes per site and one bit.
constexpr int CS_THREADS = 256, CS_LANES = CS_THREADS / 4, CS_PLANES = 8, CS_CHUNK = 255, CS_CATS = 5, CS_PARTIAL = 10;

__global__ __launch_bounds__(CS_THREADS) void site_census_kernel(const unsigned *__restrict__ P, size_t n, size_t n_pad, size_t L,
                                                                 unsigned *__restrict__ counts, unsigned *__restrict__ differs)
{
    __shared__ __align__(16) unsigned sh[CS_PLANES][4][CS_LANES];
    __shared__ unsigned half_sum[CS_CATS][128];
    __shared__ unsigned sh_pres[CS_PARTIAL][4];
    const size_t g = blockIdx.x;
    const unsigned t = threadIdx.x;
    const unsigned *__restrict__ Pg = P + g * NPLANES * n_pad * 4;       // (dwords: sample s, word q of plane p at (p * n_pad + s) * 4 + q)
    const size_t plane = n_pad * 4;
    const unsigned q = t & 3u, sl = t >> 2;
    const unsigned site = t & 127u, w = site >> 5, bit = site & 31u, half = t >> 7;
    if (t < CS_PARTIAL * 4) (&sh_pres[0][0])[t] = 0u;
    unsigned total[CS_CATS];
#pragma unroll
    for (int c = 0; c < CS_CATS; c++) total[c] = 0;
    unsigned pres[CS_PARTIAL];
#pragma unroll
    for (int m = 0; m < CS_PARTIAL; m++) pres[m] = 0;
    for (size_t s0 = 0; s0 < n; s0 += (size_t)CS_LANES * CS_CHUNK) {
        const size_t s1 = min(n, s0 + (size_t)CS_LANES * CS_CHUNK);
        unsigned cnt[CS_CATS][CS_PLANES];
#pragma unroll
        for (int c = 0; c < CS_CATS; c++)
#pragma unroll
            for (int k = 0; k < CS_PLANES; k++) cnt[c][k] = 0;
#pragma unroll 2
        for (size_t s = s0 + sl; s < s1; s += CS_LANES) {
            const size_t o = s * 4 + q;
            const unsigned a = Pg[o], c = Pg[plane + o], gg = Pg[2 * plane + o], tt = Pg[3 * plane + o];
            // minterms of (a, c) and of (g, t): index = bit 0 | bit 1 << 1
            const unsigned ac[4] = {~(a | c), a & ~c, ~a & c, a & c};
            const unsigned gt[4] = {~(gg | tt), gg & ~tt, ~gg & tt, gg & tt};
            // mask = ac index | gt index << 2.  One-hot: A = 1, C = 2, G = 4, T = 8; N = 15
            const unsigned cat[CS_CATS] = {ac[1] & gt[0], ac[2] & gt[0], ac[0] & gt[1], ac[0] & gt[2], ac[3] & gt[3]};
#pragma unroll
            for (int k5 = 0; k5 < CS_CATS; k5++) {
                unsigned carry = cat[k5];
#pragma unroll
                for (int k = 0; k < CS_PLANES; k++) {
                    const unsigned nc = cnt[k5][k] & carry;
                    cnt[k5][k] ^= carry;
                    carry = nc;
                }
            }
            // the ten partial codes in the order of their mask: 3, 5, 6, 7, 9, 10, 11, 12, 13, 14
            pres[0] |= ac[3] & gt[0];
            pres[1] |= ac[1] & gt[1];
            pres[2] |= ac[2] & gt[1];
            pres[3] |= ac[3] & gt[1];
            pres[4] |= ac[1] & gt[2];
            pres[5] |= ac[2] & gt[2];
            pres[6] |= ac[3] & gt[2];
            pres[7] |= ac[0] & gt[3];
            pres[8] |= ac[1] & gt[3];
            pres[9] |= ac[2] & gt[3];
        }
        // planes in use (workgroup-uniform): enough bits for the most samples any lane added in this chunk
        const unsigned iters = (unsigned)((s1 - s0 + CS_LANES - 1) / CS_LANES);
        const int K = 32 - __clz(iters);
#pragma unroll
        for (int c = 0; c < CS_CATS; c++) {
#pragma unroll
            for (int k = 0; k < CS_PLANES; k++)
                if (k < K) sh[k][q][sl] = cnt[c][k];
            __syncthreads();
            unsigned sum = 0;
            for (int k = 0; k < K; k++) {
                const uint4 *__restrict__ row = reinterpret_cast<const uint4 *>(&sh[k][w][half * 32u]);
                unsigned acc = 0;
#pragma unroll
                for (int l = 0; l < 8; l++) {
                    const uint4 v = row[l];
                    acc += ((v.x >> bit) & 1u) + ((v.y >> bit) & 1u) + ((v.z >> bit) & 1u) + ((v.w >> bit) & 1u);
                }
                sum += acc << k;
            }
            total[c] += sum;
            __syncthreads();
        }
    }
    // presence of the partial codes: OR over the lanes of the wave that hold the same word (lane & 3), then over the waves
#pragma unroll
    for (int m = 0; m < CS_PARTIAL; m++) {
        unsigned v = pres[m];
#pragma unroll
        for (int off = 32; off >= 4; off >>= 1) v |= __shfl_xor(v, off, 64);
        if ((t & 63u) < 4u && v) atomicOr(&sh_pres[m][q], v);
    }
    if (half)
#pragma unroll
        for (int c = 0; c < CS_CATS; c++) half_sum[c][site] = total[c];
    __syncthreads();
    if (half) return;                                      // (threads 0 .. 127: two whole waves stay)
    const size_t abs_site = g * SITES_PER_GROUP + site;
    const bool valid = abs_site < L;
    unsigned sum5 = 0;
#pragma unroll
    for (int c = 0; c < CS_CATS; c++) {
        total[c] += half_sum[c][site];
        sum5 += total[c];
    }
    // presence bit = mask - 1: the one-hot masks 1, 2, 4, 8 from their counts, the partial codes from their words
    unsigned presence = (total[0] ? 1u : 0u) | (total[1] ? 2u : 0u) | (total[2] ? 8u : 0u) | (total[3] ? 128u : 0u);
    const unsigned partial_bit[CS_PARTIAL] = {2, 4, 5, 6, 8, 9, 10, 11, 12, 13};
#pragma unroll
    for (int m = 0; m < CS_PARTIAL; m++) presence |= ((sh_pres[m][w] >> bit) & 1u) << partial_bit[m];
    const bool d = valid && ((g_differs_table[presence >> 5] >> (presence & 31u)) & 1u);
    const unsigned long long b = __ballot(d);
    if ((t & 63u) == 0) {
        differs[g * 4 + (t >> 6) * 2] = (unsigned)b;
        differs[g * 4 + (t >> 6) * 2 + 1] = (unsigned)(b >> 32);
    }
    if (valid && counts != nullptr) {
#pragma unroll
        for (int c = 0; c < CS_CATS; c++) counts[(size_t)c * L + abs_site] = total[c];
        counts[(size_t)CS_CATS * L + abs_site] = (unsigned)n - sum5;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Unpack: the transpose through LDS.  One workgroup = 64 samples x one group of 128 sites.  Load: wave p reads plane p (A, C, G, T)
// of the 64 samples, one uint4 per lane -- 1 KiB per wave, coalesced -- into LDS as [plane][sample].  Store: thread t writes the 16
// bytes of sites [16 (t & 7), +16) of row t >> 3 (and of row 32 + (t >> 3) in a second pass), so eight neighbouring lanes store one
// whole 128-byte run of one row -- a full line when the row is aligned -- where the plain form (one thread per (sample, group), the
// inverse of pack_kernel) has every lane of a wave in a row of its own, 64 lines per store instruction.  Writes are two thirds of
// this kernel's traffic, so they decide.  The LDS reads of a wave are four bytes per lane at [plane][8 rows][word (t & 7) >> 1]: 32
// different consecutive dwords, each read by two lanes (a broadcast) -- one bank each, no conflict; the writes are 16 bytes per lane,
// consecutive.  The 16-byte store needs the row's address aligned and all 16 columns inside L; everything else goes byte by byte
// under `column < L`.  Rows outside [first, first + count), pad samples, tail bits and pad groups are neither loaded nor stored.
// Reads 64 bytes per sample and group (0.5 B per site), writes 1 B per sample and site.
__device__ __forceinline__ unsigned iupac_letter(unsigned m)
{
    //                                        "VSRGMCAX"                 "NBDKHYWT"
    const unsigned long long lo = 0x565352474D434158ull, hi = 0x4E42444B48595754ull;
    return (unsigned)(((m < 8u ? lo : hi) >> ((m & 7u) * 8u)) & 0xFFull);
}

__global__ __launch_bounds__(256) void unpack_kernel(const uint4 *__restrict__ P, size_t n_pad, size_t L, size_t first, size_t count,
                                                     unsigned block_y0, uint8_t *__restrict__ ascii, size_t stride)
{
    __shared__ uint4 sh[4][64];
    const size_t g = blockIdx.x;
    const size_t k0 = ((size_t)block_y0 + blockIdx.y) * 64;             // first row of this workgroup
    const unsigned t = threadIdx.x;
    {
        const unsigned p = t >> 6, lane = t & 63u;
        const size_t k = k0 + lane;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (k < count) v = P[(g * NPLANES + p) * n_pad + first + k];
        sh[p][lane] = v;
    }
    __syncthreads();
    const unsigned seg = t & 7u;
    const size_t col0 = g * SITES_PER_GROUP + seg * 16u;
    if (col0 >= L) return;
    const unsigned shift = (seg & 1u) * 16u, word = seg >> 1;
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const unsigned r = pass * 32u + (t >> 3);
        const size_t k = k0 + r;
        if (k >= count) continue;
        unsigned x[4];
#pragma unroll
        for (int p = 0; p < 4; p++) x[p] = (reinterpret_cast<const unsigned *>(&sh[p][r])[word] >> shift) & 0xFFFFu;
        unsigned out[4];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            unsigned o = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const unsigned i = d * 4 + b;
                const unsigned m = ((x[0] >> i) & 1u) | (((x[1] >> i) & 1u) << 1) | (((x[2] >> i) & 1u) << 2) | (((x[3] >> i) & 1u) << 3);
                o |= iupac_letter(m) << (8 * b);
            }
            out[d] = o;
        }
        uint8_t *dst = ascii + k * stride + col0;
        if (col0 + 16 <= L && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
            *reinterpret_cast<uint4 *>(dst) = make_uint4(out[0], out[1], out[2], out[3]);
        } else {
            const unsigned nb = (unsigned)min((size_t)16, L - col0);
#pragma unroll
            for (unsigned b = 0; b < 16; b++)
                if (b < nb) dst[b] = (uint8_t)(out[b >> 2] >> (8 * (b & 3u)));
        }
    }
}

// counts (device, may be NULL) and the differs bitmap into `differs_d` (device, 4 words per group)
static int launch_census(const tracs_alignment *a, unsigned *counts, unsigned *differs_d, hipStream_t stream)
{
    TRACS_HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_differs_table), differs_table(), DIFFERS_WORDS * 4, 0, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(site_census_kernel, dim3((unsigned)a->groups), dim3(CS_THREADS), 0, stream, reinterpret_cast<const unsigned *>(a->planes), a->n, a->n_pad, a->L,
                       counts, differs_d);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

int site_census(const tracs_alignment *a, uint32_t *counts, uint64_t *differs, size_t *n_differs, hipStream_t stream)
{
    if (n_differs) *n_differs = 0;
    if (!a) { set_error("tracs_alignment_site_census: NULL argument"); return TRACS_E_ARG; }
    if (!a->L) return TRACS_OK;
    DeviceCall guard(stream);
    const size_t words64 = (a->L + 63) / 64;
    if (!a->n) {
        if (counts) TRACS_HIP_CHECK(hipMemsetAsync(counts, 0, a->L * 6 * 4, stream));
        if (differs) std::memset(differs, 0, words64 * 8);
        return TRACS_OK;
    }
    unsigned *d = nullptr;                                      // the differs bitmap on the device, 4 words per group
    int rc = workspace_get(WS_MSA_DIFFERS, a->groups * 4, &d);
    if (rc) return rc;
    if ((rc = launch_census(a, counts, d, stream))) return rc;
    if (differs || n_differs) {
        std::vector<uint64_t> tmp;
        uint64_t *dst = differs;
        if (!dst) { tmp.resize(words64); dst = tmp.data(); }
        TRACS_HIP_CHECK(hipMemcpyAsync(dst, d, words64 * 8, hipMemcpyDeviceToHost, stream));
        TRACS_HIP_CHECK(hipStreamSynchronize(stream));
        size_t pop = 0;
        for (size_t w = 0; w < words64; w++) pop += (size_t)__builtin_popcountll(dst[w]);
        if (n_differs) *n_differs = pop;
    }
    return TRACS_OK;
}

int unpack_rows(const tracs_alignment *a, size_t first, size_t count, uint8_t *ascii, size_t stride, hipStream_t stream)
{
    if (!a || !ascii) { set_error("tracs_alignment_unpack: NULL argument"); return TRACS_E_ARG; }
    if (first > a->n || count > a->n - first) { set_error("tracs_alignment_unpack: sample range outside the alignment"); return TRACS_E_ARG; }
    if (stride < a->L) { set_error("tracs_alignment_unpack: stride shorter than one row"); return TRACS_E_ARG; }
    if (!count || !a->L) return TRACS_OK;
    DeviceCall guard(stream);
    const size_t blocks_y = (count + 63) / 64, slice = 65535;
    for (size_t y0 = 0; y0 < blocks_y; y0 += slice) {
        const dim3 grid((unsigned)a->groups, (unsigned)std::min(slice, blocks_y - y0));
        hipLaunchKernelGGL(unpack_kernel, grid, dim3(256), 0, stream, a->planes, a->n_pad, a->L, first, count, (unsigned)y0, ascii, stride);
    }
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

}  // namespace tracs

using namespace tracs;

extern "C" {

int tracs_alignment_site_census(const tracs_alignment *a, uint32_t *counts, uint64_t *differs, size_t *n_differs, void *stream)
{
    return site_census(a, counts, differs, n_differs, static_cast<hipStream_t>(stream));
}

int tracs_alignment_unpack(const tracs_alignment *a, size_t first, size_t count, uint8_t *ascii, size_t stride, void *stream)
{
    return unpack_rows(a, first, count, ascii, stride, static_cast<hipStream_t>(stream));
}

// host-only (tests): the differs table, 2^14 bits = 2 048 bytes, bit p of byte p / 8
int tracs_debug_differs_table(uint8_t *out, size_t bytes)
{
    if (!out || bytes < DIFFERS_WORDS * 4) { set_error("tracs_debug_differs_table: 2048 bytes"); return TRACS_E_ARG; }
    std::memcpy(out, differs_table(), DIFFERS_WORDS * 4);
    return TRACS_OK;
}

}  // extern "C"
