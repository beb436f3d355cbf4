// site_select.hip -- site rules: which columns of a packed alignment feed the pair matrix.
//
// A run with a site rule is, by definition, the run on the alignment with the dropped columns deleted from every record.  So the
// rule is applied once, to the packed planes: the kept columns are packed into a NEW handle that is byte for byte what packing the
// column-deleted text gives, and everything downstream (pair kernels, site classes, lists, the recombination filter) runs on that
// handle unchanged.
//
//     site_n_count_kernel    per site: the samples whose stored N bit is set there (one read of plane 4 of every group)
//     keep_bits_kernel       the final keep bitmap: the caller's bitmap AND [N count <= max_n_samples] AND [site < L]
//     word_offsets_kernel    exclusive prefix sums of the bitmap's 32-site words (the rank of each word's first kept site)
//     site_list_kernel       the kept sites in order (what an output group's first and last site are looked up in)
//     select_sites_kernel    the five planes of the kept sites
#include "common.h"
#include "debug_api.h"

#include <algorithm>
#include <cstring>
#include <string>

namespace tracs {

// ---------------------------------------------------------------------------------------------------------------------------------
// N samples per site.  One workgroup = one group of 128 sites, lanes over samples as in classify_sites_kernel (a wave's load of one
// (group, plane 4) run is 1 KiB, coalesced).  Every lane adds its samples' 128 N bits into bit-sliced counters -- NC_PLANES words of
// 32 one-bit columns per 32-site word, a ripple-carry add per loaded word -- so a loaded uint4 costs ~16 VALU operations per word
// instead of the 32 ballots per word that counting per bit column takes.  The counters are flushed through LDS once per 255 samples
// per lane: thread t sums bit (t & 31) of word (t >> 5) & 3 over the lanes of its half of the workgroup (the LDS reads of a wave are
// two broadcast addresses).  Reads plane 4 once: n_pad x groups x 16 bytes, 1 / 5 of the planes; writes 4 bytes per site.
constexpr int NC_THREADS = 256, NC_PLANES = 8, NC_CHUNK = 255;

__global__ __launch_bounds__(NC_THREADS) void site_n_count_kernel(const uint4 *__restrict__ P, size_t n_pad, size_t L, unsigned *__restrict__ counts)
{
    __shared__ unsigned sh[NC_PLANES][4][NC_THREADS];
    __shared__ unsigned half_sum[128];
    const size_t g = blockIdx.x;
    const unsigned t = threadIdx.x;
    const uint4 *__restrict__ Ng = P + (g * NPLANES + 4) * n_pad;
    const unsigned site = t & 127u, w = site >> 5, bit = site & 31u, half = t >> 7;
    unsigned total = 0;
    for (size_t s0 = 0; s0 < n_pad; s0 += (size_t)NC_THREADS * NC_CHUNK) {
        const size_t s1 = min(n_pad, s0 + (size_t)NC_THREADS * NC_CHUNK);
        unsigned c[NC_PLANES][4];
#pragma unroll
        for (int k = 0; k < NC_PLANES; k++)
#pragma unroll
            for (int q = 0; q < 4; q++) c[k][q] = 0;
        for (size_t s = s0 + t; s < s1; s += NC_THREADS) {
            const uint4 v = Ng[s];
            const unsigned x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                unsigned carry = x[q];
#pragma unroll
                for (int k = 0; k < NC_PLANES; k++) {
                    const unsigned nc = c[k][q] & carry;
                    c[k][q] ^= carry;
                    carry = nc;
                }
            }
        }
        // planes in use (workgroup-uniform): enough bits for the most samples any lane added in this chunk
        const unsigned iters = (unsigned)((s1 - s0 + NC_THREADS - 1) / NC_THREADS);
        const int K = 32 - __clz(iters);
#pragma unroll
        for (int k = 0; k < NC_PLANES; k++)
            if (k < K)
#pragma unroll
                for (int q = 0; q < 4; q++) sh[k][q][t] = c[k][q];
        __syncthreads();
        for (int k = 0; k < K; k++) {
            const uint4 *__restrict__ row = reinterpret_cast<const uint4 *>(&sh[k][w][half * 128u]);
            unsigned acc = 0;
#pragma unroll 4
            for (int l = 0; l < 32; l++) {
                const uint4 v = row[l];
                acc += ((v.x >> bit) & 1u) + ((v.y >> bit) & 1u) + ((v.z >> bit) & 1u) + ((v.w >> bit) & 1u);
            }
            total += acc << k;
        }
        __syncthreads();
    }
    if (half) half_sum[site] = total;
    __syncthreads();
    const size_t abs_site = g * SITES_PER_GROUP + site;
    if (!half && abs_site < L) counts[abs_site] = total + half_sum[site];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The final bitmap, one thread per site: kept = [site < L] AND the caller's bit AND [N count <= max_n].  words = 4 per group.
__global__ __launch_bounds__(256) void keep_bits_kernel(const unsigned *__restrict__ keep_in, const unsigned *__restrict__ counts, unsigned max_n,
                                                        size_t L, size_t words, unsigned *__restrict__ keepw)
{
    const size_t site = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool ok = site < L;
    if (ok && keep_in != nullptr) ok = (keep_in[site >> 5] >> (site & 31u)) & 1u;
    if (ok && counts != nullptr) ok = counts[site] <= max_n;
    const unsigned long long b = __ballot(ok);
    const size_t w = site >> 5;
    if ((threadIdx.x & 63u) == 0 && w < words) { keepw[w] = (unsigned)b; keepw[w + 1] = (unsigned)(b >> 32); }
}

// exclusive prefix sums of the words' populations (one workgroup, 1 024 words per step: group_offsets_kernel's scan), total[0] = kept sites
__global__ __launch_bounds__(1024) void word_offsets_kernel(const unsigned *__restrict__ keepw, size_t words, unsigned *__restrict__ woff,
                                                            unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long wave_tot[2][16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long base = 0;
    int par = 0;
    for (size_t w0 = 0; w0 < words; w0 += 1024, par ^= 1) {
        const size_t w = w0 + t;
        const unsigned long long c = w < words ? (unsigned long long)__popc(keepw[w]) : 0ull;
        unsigned long long incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wave_tot[par][wave] = incl;
        __syncthreads();                                  // (wave_tot[par ^ 1] was last read before the previous step's barrier)
        unsigned long long before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) { const unsigned long long v = wave_tot[par][k]; if (k < wave) before += v; all += v; }
        if (w < words) woff[w] = (unsigned)(base + before + incl - c);
        base += all;
    }
    if (t == 0) total[0] = base;
}

// the kept sites in site order: list[woff[w] ..] = the set bits of word w
__global__ __launch_bounds__(256) void site_list_kernel(const unsigned *__restrict__ keepw, const unsigned *__restrict__ woff, size_t words,
                                                        unsigned *__restrict__ list)
{
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    unsigned x = keepw[w], o = woff[w];
    while (x) {
        list[o++] = (unsigned)(w * 32 + (__ffs(x) - 1));
        x &= x - 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// compress (Hacker's Delight 7-4): the bits of x under mask m, moved to the low end in order.  The five move masks depend on m alone;
// m is wave-uniform here, so they are computed once per source word on the scalar unit, and a word costs each lane and plane 5 x 4
// operations.
struct CompressMasks { unsigned m, mv[5]; };
__device__ __forceinline__ CompressMasks compress_masks(unsigned m)
{
    CompressMasks r;
    r.m = m;
    unsigned mk = ~m << 1;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        unsigned mp = mk ^ (mk << 1);
        mp ^= mp << 2; mp ^= mp << 4; mp ^= mp << 8; mp ^= mp << 16;
        const unsigned mv = mp & m;
        r.mv[i] = mv;
        m = (m ^ mv) | (mv >> (1 << i));
        mk &= ~mp;
    }
    return r;
}
__device__ __forceinline__ unsigned compress_apply(unsigned x, const CompressMasks &cm)
{
    x &= cm.m;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const unsigned t = x & cm.mv[i];
        x = (x ^ t) | (t >> (1 << i));
    }
    return x;
}

// Select: one thread = one (sample, OUTPUT group of 128 kept sites), lanes over samples like pack_kernel and compact_sites_kernel, so
// every source site, mask and shift is wave-uniform.  An output group's kept sites lie in the source groups [g0, g1] (from the list).
//   stream  (at least one kept site per source group of the span on average): every source group of the span that keeps anything is
//           loaded whole -- five 16-byte loads per lane, 1 KiB per wave and plane --, each of its four words is compressed under its
//           keep mask (not at all where the mask is full) and appended to a 64-bit accumulator per plane; every 32 bits an output word
//           is complete.  A source group that two output groups share is loaded by both: the second read comes from the cache, the
//           two waves are neighbours in one workgroup.
//   gather  (sparser): the words of the listed sites one dword per lane, eight sites in flight, bit by bit -- compact_sites_kernel's
//           scattered branch; streaming would load groups that keep nothing.
// Reads what it keeps (5 x 16 bytes per sample and source group with a kept site), writes 5 x 16 bytes per sample and output group;
// tail bits of the last group stay zero, pad samples are not written (the handle was cleared when it was created).
__global__ __launch_bounds__(256) void select_sites_kernel(const uint4 *__restrict__ src, const unsigned *__restrict__ list, unsigned count,
                                                           const uint4 *__restrict__ keepw, const uint4 *__restrict__ woff,
                                                           uint4 *__restrict__ dst, size_t n_pad, unsigned s_first, unsigned n, unsigned groups_dst)
{
    const unsigned s = s_first + blockIdx.y * 64 + (threadIdx.x & 63);
    const unsigned G = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (G >= groups_dst || s >= n_pad) return;
    const unsigned pos0 = G * SITES_PER_GROUP;
    const unsigned kn = min((unsigned)SITES_PER_GROUP, count - pos0);
    const unsigned first = __builtin_amdgcn_readfirstlane(list[pos0]), last = __builtin_amdgcn_readfirstlane(list[pos0 + kn - 1]);
    const unsigned g0 = first >> 7, g1 = last >> 7;
    unsigned out[NPLANES][4];
#pragma unroll
    for (int p = 0; p < NPLANES; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) out[p][q] = 0;
    if (g1 - g0 + 1 > kn) {
        const unsigned *__restrict__ srcw = reinterpret_cast<const unsigned *>(src);
        for (unsigned ow = 0; ow < 4; ow++) {                            // (wave-uniform; out[][] is only ever indexed by constants)
            const unsigned tb = pos0 + ow * 32;
            const unsigned kw = tb >= count ? 0u : min(32u, count - tb);
            unsigned accw[NPLANES];
#pragma unroll
            for (int p = 0; p < NPLANES; p++) accw[p] = 0;
            for (unsigned k0 = 0; k0 < kw; k0 += 8) {
                unsigned site[8], in[8][NPLANES];
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    site[q] = __builtin_amdgcn_readfirstlane(list[tb + min(k0 + q, kw - 1u)]);
#pragma unroll
                    for (int p = 0; p < NPLANES; p++)
                        in[q][p] = srcw[(((size_t)(site[q] >> 7) * NPLANES + p) * n_pad + s) * 4 + ((site[q] >> 5) & 3u)];
                }
#pragma unroll
                for (int q = 0; q < 8; q++)
                    if (k0 + q < kw)                                      // (wave-uniform)
#pragma unroll
                        for (int p = 0; p < NPLANES; p++) accw[p] |= ((in[q][p] >> (site[q] & 31u)) & 1u) << (k0 + q);
            }
#pragma unroll
            for (int p = 0; p < NPLANES; p++) {
#pragma unroll
                for (int q = 0; q < 4; q++) out[p][q] = ow == (unsigned)q ? accw[p] : out[p][q];
            }
        }
    } else {
        unsigned long long acc[NPLANES];
#pragma unroll
        for (int p = 0; p < NPLANES; p++) acc[p] = 0;
        unsigned fill = 0, ow = 0;                                        // wave-uniform: bits waiting in acc, output words done
        auto emit = [&]() {
#pragma unroll
            for (int p = 0; p < NPLANES; p++) {
                const unsigned v = (unsigned)acc[p];
#pragma unroll
                for (int q = 0; q < 4; q++) out[p][q] = ow == (unsigned)q ? v : out[p][q];      // (selects: a store under a branch would index out[][])
            }
        };
        for (unsigned g = g0; g <= g1; g++) {
            const uint4 m4 = keepw[g];
            const unsigned m[4] = {(unsigned)__builtin_amdgcn_readfirstlane(m4.x), (unsigned)__builtin_amdgcn_readfirstlane(m4.y),
                                   (unsigned)__builtin_amdgcn_readfirstlane(m4.z), (unsigned)__builtin_amdgcn_readfirstlane(m4.w)};
            if ((m[0] | m[1] | m[2] | m[3]) == 0u) continue;
            const uint4 o4 = woff[g];
            const unsigned o[4] = {(unsigned)__builtin_amdgcn_readfirstlane(o4.x), (unsigned)__builtin_amdgcn_readfirstlane(o4.y),
                                   (unsigned)__builtin_amdgcn_readfirstlane(o4.z), (unsigned)__builtin_amdgcn_readfirstlane(o4.w)};
            uint4 v[NPLANES];
#pragma unroll
            for (int p = 0; p < NPLANES; p++) v[p] = src[((size_t)g * NPLANES + p) * n_pad + s];
            // one source word: mask mk, rank ok of its first kept site, the word of each plane
            auto take = [&](unsigned mk, unsigned ok, unsigned x0, unsigned x1, unsigned x2, unsigned x3, unsigned x4) {
                const unsigned c = __popc(mk);
                // the word's kept sites have the ranks [ok, ok + c); this group takes the ranks [pos0, pos0 + kn)
                if (mk == 0u || ok + c <= pos0 || ok >= pos0 + kn) return;
                const unsigned skip = ok < pos0 ? pos0 - ok : 0u;
                const unsigned nb = min(ok + c, pos0 + kn) - (ok + skip);
                const unsigned low = nb == 32u ? 0xFFFFFFFFu : ((1u << nb) - 1u);
                unsigned x[NPLANES] = {x0, x1, x2, x3, x4};
                if (mk != 0xFFFFFFFFu) {                                  // (wave-uniform)
                    const CompressMasks cm = compress_masks(mk);
#pragma unroll
                    for (int p = 0; p < NPLANES; p++) x[p] = compress_apply(x[p], cm);
                }
#pragma unroll
                for (int p = 0; p < NPLANES; p++) acc[p] |= (unsigned long long)((x[p] >> skip) & low) << fill;
                fill += nb;
                if (fill >= 32u) {
                    emit();
#pragma unroll
                    for (int p = 0; p < NPLANES; p++) acc[p] >>= 32;
                    fill -= 32u;
                    ow++;
                }
            };
            take(m[0], o[0], v[0].x, v[1].x, v[2].x, v[3].x, v[4].x);
            take(m[1], o[1], v[0].y, v[1].y, v[2].y, v[3].y, v[4].y);
            take(m[2], o[2], v[0].z, v[1].z, v[2].z, v[3].z, v[4].z);
            take(m[3], o[3], v[0].w, v[1].w, v[2].w, v[3].w, v[4].w);
        }
        if (fill) emit();
    }
    if (s < n)
#pragma unroll
        for (int p = 0; p < NPLANES; p++)
            dst[((size_t)G * NPLANES + p) * n_pad + s] = make_uint4(out[p][0], out[p][1], out[p][2], out[p][3]);
}

static void launch_n_counts(const tracs_alignment *a, unsigned *counts, hipStream_t stream)
{
    hipLaunchKernelGGL(site_n_count_kernel, dim3((unsigned)a->groups), dim3(NC_THREADS), 0, stream, a->planes, a->n_pad, a->L, counts);
}

void launch_compact_general(const uint4 *src, const unsigned *list, unsigned count, uint4 *dst, size_t n_pad, unsigned n, unsigned groups_dst,
                            hipStream_t stream);      // site_classes.hip

// the temporaries of one selection, one device block: [N counts] [caller's bitmap] final bitmap, word offsets, the total, the list
struct Selection {
    DeviceArray<uint8_t> tmp;
    unsigned *counts = nullptr, *keep_in = nullptr, *keepw = nullptr, *woff = nullptr, *list = nullptr;
    unsigned long long *total_d = nullptr;
    size_t words = 0, words64 = 0;
    uint32_t max_n = UINT32_MAX;
};

static int selection_alloc(const tracs_alignment *src, bool has_keep, uint32_t max_n, Selection &sel)
{
    const size_t L = src->L;
    sel.words = src->groups * 4;
    sel.words64 = (L + 63) / 64;
    sel.max_n = max_n;
    const bool n_rule = max_n != UINT32_MAX;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_counts = n_rule ? up(L * 4) : 0, b_in = has_keep ? up(sel.words * 4) : 0, b_words = up(sel.words * 4), b_list = up(L * 4);
    if (const int rc = sel.tmp.alloc(b_counts + b_in + 2 * b_words + 256 + b_list, "site selection")) return rc;
    uint8_t *p = sel.tmp.get();
    if (n_rule) sel.counts = reinterpret_cast<unsigned *>(p);
    p += b_counts;
    if (has_keep) sel.keep_in = reinterpret_cast<unsigned *>(p);
    p += b_in;
    sel.keepw = reinterpret_cast<unsigned *>(p); p += b_words;
    sel.woff = reinterpret_cast<unsigned *>(p); p += b_words;
    sel.total_d = reinterpret_cast<unsigned long long *>(p); p += 256;
    sel.list = reinterpret_cast<unsigned *>(p);
    return TRACS_OK;
}

static hipError_t selection_upload(const Selection &sel, const uint64_t *keep, hipStream_t stream)
{
    if (!sel.keep_in) return hipSuccess;
    hipError_t e = hipMemsetAsync(sel.keep_in, 0, sel.words * 4, stream);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(sel.keep_in, keep, sel.words64 * 8, hipMemcpyHostToDevice, stream);
}

static void selection_bitmap(const tracs_alignment *src, const Selection &sel, hipStream_t stream)
{
    hipLaunchKernelGGL(keep_bits_kernel, dim3((unsigned)((sel.words * 32 + 255) / 256)), dim3(256), 0, stream, sel.keep_in, sel.counts, sel.max_n, src->L,
                       sel.words, sel.keepw);
    hipLaunchKernelGGL(word_offsets_kernel, dim3(1), dim3(1024), 0, stream, sel.keepw, sel.words, sel.woff, sel.total_d);
}

static void selection_list(const Selection &sel, hipStream_t stream)
{
    hipLaunchKernelGGL(site_list_kernel, dim3((unsigned)((sel.words + 255) / 256)), dim3(256), 0, stream, sel.keepw, sel.woff, sel.words, sel.list);
}

static void selection_pack(const tracs_alignment *src, const Selection &sel, unsigned total, tracs_alignment *dst, hipStream_t stream)
{
    const unsigned groups_dst = (unsigned)dst->groups;
    const size_t blocks_y = src->n_pad / 64, slice = 65535;
    for (size_t y0 = 0; y0 < blocks_y; y0 += slice) {
        const dim3 grid((groups_dst + 3) / 4, (unsigned)std::min(slice, blocks_y - y0));
        hipLaunchKernelGGL(select_sites_kernel, grid, dim3(256), 0, stream, src->planes, sel.list, total, reinterpret_cast<const uint4 *>(sel.keepw),
                           reinterpret_cast<const uint4 *>(sel.woff), dst->planes, src->n_pad, (unsigned)(y0 * 64), (unsigned)src->n, groups_dst);
    }
}

static int selection_check_args(const tracs_alignment *src, const uint64_t *keep, size_t keep_len)
{
    if (keep && keep_len != src->L) {
        set_error("site rules: the keep bitmap covers " + std::to_string(keep_len) + " sites, the alignment has " + std::to_string(src->L));
        return TRACS_E_ARG;
    }
    if (!src->L || !src->n) { set_error("no site left after the site rules"); return TRACS_E_ARG; }
    return TRACS_OK;
}

// the kept sites of `src` packed into a new handle (include/tracs_hip.h: tracs_alignment_select_sites).  release_src_arena: the caller
// frees `src` right afterwards (the FASTA entry points), so its arena -- nothing has been built in it yet -- goes before the new
// handle's planes and arena are allocated: the peak is source planes + new planes + one arena.
int select_sites(tracs_alignment *src, const uint64_t *keep, size_t keep_len, uint32_t max_n_samples, tracs_alignment **out,
                 uint64_t *kept, size_t *n_kept, hipStream_t stream, bool release_src_arena)
{
    if (out) *out = nullptr;
    if (n_kept) *n_kept = 0;
    if (!src || !out) { set_error("tracs_alignment_select_sites: NULL argument"); return TRACS_E_ARG; }
    int rc = selection_check_args(src, keep, keep_len);
    if (rc) return rc;
    DeviceCall guard(stream);
    Selection sel;
    if ((rc = selection_alloc(src, keep != nullptr, max_n_samples, sel))) return rc;
    TRACS_HIP_CHECK(selection_upload(sel, keep, stream));
    if (sel.counts) launch_n_counts(src, sel.counts, stream);
    selection_bitmap(src, sel, stream);
    TRACS_HIP_CHECK(hipGetLastError());
    unsigned long long total = 0;
    TRACS_HIP_CHECK(hipMemcpyAsync(&total, sel.total_d, 8, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    if (total == 0) { set_error("no site left after the site rules"); return TRACS_E_ARG; }
    selection_list(sel, stream);
    if (release_src_arena && src->arena && src->arena_used == 0 && src->pack_extra.empty()) {
        device_free(src->arena);
        src->arena = nullptr;
        src->arena_bytes = 0;
    }
    tracs_alignment *made = nullptr;
    if ((rc = tracs_alignment_create(src->n, (size_t)total, &made))) return rc;
    AlignmentOwner dst(made);
    TRACS_HIP_CHECK(hipStreamSynchronize(nullptr));              // the new planes are cleared on the null stream
    selection_pack(src, sel, (unsigned)total, dst.get(), stream);
    TRACS_HIP_CHECK(hipGetLastError());
    if (kept) TRACS_HIP_CHECK(hipMemcpyAsync(kept, sel.keepw, sel.words64 * 8, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    if (n_kept) *n_kept = (size_t)total;
    *out = dst.release();
    return TRACS_OK;
}

}  // namespace tracs

using namespace tracs;

extern "C" {

int tracs_alignment_site_n_counts(const tracs_alignment *a, uint32_t *counts, void *stream_)
{
    if (!a || (!counts && a->L)) { set_error("tracs_alignment_site_n_counts: NULL argument"); return TRACS_E_ARG; }
    if (!a->L) return TRACS_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceCall guard(stream);
    if (!a->n) { TRACS_HIP_CHECK(hipMemsetAsync(counts, 0, a->L * 4, stream)); return TRACS_OK; }
    launch_n_counts(a, counts, stream);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

int tracs_alignment_select_sites(const tracs_alignment *src, const uint64_t *keep, size_t keep_len, uint32_t max_n_samples,
                                 tracs_alignment **out, uint64_t *kept, size_t *n_kept, void *stream)
{
    return select_sites(const_cast<tracs_alignment *>(src), keep, keep_len, max_n_samples, out, kept, n_kept, static_cast<hipStream_t>(stream), false);
}

// Measurement (scripts/bench_sites.py): the stages of one selection between HIP events, `repeats` times after one warm-up round, and
// the same list through the re-pack kernel of the site classes (compact_sites_kernel<0>) in alternation with select_sites_kernel.
// ms: [repeats][4] = N count (0 without the N rule), bitmap + offsets + list, select_sites_kernel, compact_sites_kernel<0>.
// *same: 1 when both kernels left the same bytes.  The selected handle is freed again.
int tracs_debug_site_select_timing(const tracs_alignment *src, const uint64_t *keep, size_t keep_len, uint32_t max_n_samples, int repeats,
                                   float *ms, size_t *n_kept, int *same)
{
    if (!src || !ms || repeats < 1) { set_error("tracs_debug_site_select_timing: bad argument"); return TRACS_E_ARG; }
    int rc = selection_check_args(src, keep, keep_len);
    if (rc) return rc;
    if (src->n_pad / 64 > 65535) { set_error("tracs_debug_site_select_timing: too many samples for the re-pack kernel"); return TRACS_E_ARG; }
    hipStream_t stream = nullptr;
    DeviceCall guard(stream);
    OwnedEvents<5> ev;
    Selection sel;
    if ((rc = selection_alloc(src, keep != nullptr, max_n_samples, sel)) || (rc = ev.create())) return rc;
    AlignmentOwner dst, dst_old;
    TRACS_HIP_CHECK(selection_upload(sel, keep, stream));
    unsigned long long total = 0;
    for (int r = -1; r < repeats; r++) {                    // r = -1: warm-up, and the round that sizes the two output handles
        TRACS_HIP_CHECK(hipEventRecord(ev[0], stream));
        if (sel.counts) launch_n_counts(src, sel.counts, stream);
        TRACS_HIP_CHECK(hipEventRecord(ev[1], stream));
        selection_bitmap(src, sel, stream);
        selection_list(sel, stream);
        TRACS_HIP_CHECK(hipEventRecord(ev[2], stream));
        if (r < 0) {
            TRACS_HIP_CHECK(hipMemcpy(&total, sel.total_d, 8, hipMemcpyDeviceToHost));
            if (total == 0) { set_error("no site left after the site rules"); return TRACS_E_ARG; }
            for (AlignmentOwner *o : {&dst, &dst_old}) {
                tracs_alignment *made = nullptr;
                if ((rc = tracs_alignment_create(src->n, (size_t)total, &made))) return rc;
                o->reset(made);
            }
            TRACS_HIP_CHECK(hipDeviceSynchronize());
            TRACS_HIP_CHECK(hipEventRecord(ev[2], stream));
        }
        selection_pack(src, sel, (unsigned)total, dst.get(), stream);
        TRACS_HIP_CHECK(hipEventRecord(ev[3], stream));
        launch_compact_general(src->planes, sel.list, (unsigned)total, dst_old->planes, src->n_pad, (unsigned)src->n, (unsigned)dst_old->groups, stream);
        TRACS_HIP_CHECK(hipEventRecord(ev[4], stream));
        TRACS_HIP_CHECK(hipGetLastError());
        TRACS_HIP_CHECK(hipEventSynchronize(ev[4]));
        if (r >= 0)
            for (int k = 0; k < 4; k++) TRACS_HIP_CHECK(hipEventElapsedTime(&ms[r * 4 + k], ev[k], ev[k + 1]));
    }
    if (same) {
        // both handles were cleared when they were created, so every byte either kernel left alone is zero in both
        const size_t bytes = tracs_alignment_bytes(dst.get());
        std::vector<uint8_t> a(std::min<size_t>(bytes, 64u << 20)), b(a.size());
        *same = 1;
        for (size_t o = 0; o < bytes && *same; o += a.size()) {
            const size_t k = std::min(a.size(), bytes - o);
            TRACS_HIP_CHECK(hipMemcpy(a.data(), reinterpret_cast<const uint8_t *>(dst->planes) + o, k, hipMemcpyDeviceToHost));
            TRACS_HIP_CHECK(hipMemcpy(b.data(), reinterpret_cast<const uint8_t *>(dst_old->planes) + o, k, hipMemcpyDeviceToHost));
            if (std::memcmp(a.data(), b.data(), k) != 0) *same = 0;
        }
    }
    if (n_kept) *n_kept = (size_t)total;
    return TRACS_OK;
}

}  // extern "C"
