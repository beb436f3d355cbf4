// sample_select.hip -- the sample rule and the pair rule: which records of a packed alignment feed the pair matrix, and
// which pairs of a dense panel were compared over enough sites.
//
// A run with the sample rule is, by definition, the run on the FASTA file(s) with the dropped records deleted.  So, like the site
// rules (site_select.hip), the rule is applied once, to the packed planes: the kept samples are gathered into a NEW handle that is byte
// for byte what packing the record-deleted text gives, and everything downstream runs on that handle unchanged.  The pair rule is one
// pass over a dense panel before any consumer reads it: a cell within the threshold whose compared-sites count is below the minimum
// becomes 0xFFFFFFFF, which every consumer already reads as "beyond the threshold, not emitted".
//
//     sample_n_count_kernel    per sample: the N bits of its stored N plane, under the file rules' bitmap where there is one
//     select_samples_kernel    the five planes of the kept samples
//     pair_min_sites_kernel    the veto pass over the cells of one dense call
#include "common.h"
#include "debug_api.h"

#include <algorithm>
#include <cstring>
#include <string>

namespace tracs {

// ---------------------------------------------------------------------------------------------------------------------------------
// N sites per sample.  Lanes over samples (a wave's load of one (group, plane 4) run is 1 KiB, coalesced), the groups split over
// blockIdx.y; every thread sums the populations of its sample's 16-byte N words -- under the group's four keep words, wave-uniform, with
// a bitmap -- and adds its partial sum to the sample's count with one integer atomic: exact in any order.  Reads plane 4 once
// (n_pad x groups x 16 bytes, 1 / 5 of the planes) and 16 bytes of bitmap per group and workgroup; writes 4 bytes per sample and
// workgroup row.  counts[] is cleared by the caller.
constexpr int SN_THREADS = 256;

template <bool MASK>
__global__ __launch_bounds__(SN_THREADS) void sample_n_count_kernel(const uint4 *__restrict__ P, size_t n_pad, unsigned n, unsigned groups,
                                                                    const uint4 *__restrict__ keepw, unsigned *__restrict__ counts)
{
    const size_t s = (size_t)blockIdx.x * SN_THREADS + threadIdx.x;
    if (s >= n_pad) return;                                              // (n_pad is a multiple of 64: whole waves leave)
    unsigned acc = 0;
    auto bits = [&](uint4 v, unsigned g) {
        if (MASK) {
            const uint4 m = keepw[g];
            v.x &= m.x; v.y &= m.y; v.z &= m.z; v.w &= m.w;
        }
        return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    };
    const unsigned step = gridDim.y;
    unsigned g = blockIdx.y;
    for (; g + 3 * (size_t)step < groups; g += 4 * step) {              // four loads in flight per lane
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = P[((size_t)(g + k * step) * NPLANES + 4) * n_pad + s];
#pragma unroll
        for (int k = 0; k < 4; k++) acc += bits(v[k], g + k * step);
    }
    for (; g < groups; g += step) acc += bits(P[((size_t)g * NPLANES + 4) * n_pad + s], g);
    if (s < n && acc) atomicAdd(&counts[s], acc);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Gather: one wave = 64 kept samples x one group, lanes over the DESTINATION samples; idx[d] = the source sample of destination d,
// ascending, so a wave's loads cover one run of (64 + the dropped samples between them) x 16 bytes per plane and its stores are 1 KiB,
// coalesced.  The groups are strided over blockIdx.x.  Reads and writes 5 x 16 bytes per kept sample and group; pad samples, pad
// groups and the slack are not written (the handle was cleared when it was created), tail bits are zero in the source.
__global__ __launch_bounds__(256) void select_samples_kernel(const uint4 *__restrict__ src, const unsigned *__restrict__ idx, uint4 *__restrict__ dst,
                                                             size_t n_pad_src, size_t n_pad_dst, unsigned n_dst, unsigned d_first, unsigned groups)
{
    const unsigned d = d_first + blockIdx.y * 64 + (threadIdx.x & 63);
    if (d >= n_dst) return;
    const size_t s = idx[d];
    for (unsigned g = blockIdx.x * 4 + (threadIdx.x >> 6); g < groups; g += gridDim.x * 4) {
        uint4 v[NPLANES];
#pragma unroll
        for (int p = 0; p < NPLANES; p++) v[p] = src[((size_t)g * NPLANES + p) * n_pad_src + s];
#pragma unroll
        for (int p = 0; p < NPLANES; p++) dst[((size_t)g * NPLANES + p) * n_pad_dst + d] = v[p];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Veto: the cells of one dense call -- rows [row_begin, row_end), columns [max(col_begin, i + 1), n) --, rows strided over
// blockIdx.y, columns over the threads.  A cell within the threshold (read unsigned) whose compared-sites count is below min_sites
// gets 0xFFFFFFFF; nothing else is written.  Reads 8 bytes per cell, writes 4 per vetoed cell.
__global__ __launch_bounds__(256) void pair_min_sites_kernel(unsigned *__restrict__ dist, const unsigned *__restrict__ ncomp, size_t ld, unsigned n,
                                                             unsigned row_begin, unsigned row_end, unsigned col_begin, unsigned thr, unsigned min_sites)
{
    for (unsigned i = row_begin + blockIdx.y; i < row_end; i += gridDim.y) {
        unsigned *__restrict__ drow = dist + (size_t)i * ld;
        const unsigned *__restrict__ nrow = ncomp + (size_t)i * ld;
        for (size_t j = (size_t)max(col_begin, i + 1) + (size_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (size_t)gridDim.x * 256)
            if (drow[j] <= thr && nrow[j] < min_sites) drow[j] = 0xFFFFFFFFu;
    }
}

static void launch_sample_counts(const tracs_alignment *a, const uint4 *keepw, unsigned *counts, hipStream_t stream)
{
    const unsigned gx = (unsigned)((a->n_pad + SN_THREADS - 1) / SN_THREADS);
    const unsigned gy = (unsigned)std::min<size_t>(std::min<size_t>(a->groups, 65535), std::max<size_t>(1, (2048 + gx - 1) / gx));
    if (keepw)
        hipLaunchKernelGGL(sample_n_count_kernel<true>, dim3(gx, gy), dim3(SN_THREADS), 0, stream, a->planes, a->n_pad, (unsigned)a->n,
                           (unsigned)a->groups, keepw, counts);
    else
        hipLaunchKernelGGL(sample_n_count_kernel<false>, dim3(gx, gy), dim3(SN_THREADS), 0, stream, a->planes, a->n_pad, (unsigned)a->n,
                           (unsigned)a->groups, keepw, counts);
}

static void launch_select_samples(const tracs_alignment *src, const unsigned *idx, tracs_alignment *dst, hipStream_t stream)
{
    const size_t waves_y = (dst->n + 63) / 64, slice = 65535;
    for (size_t y0 = 0; y0 < waves_y; y0 += slice) {
        const unsigned gy = (unsigned)std::min(slice, waves_y - y0);
        const unsigned gx = (unsigned)std::min<size_t>((src->groups + 3) / 4, std::max<size_t>(1, 8192 / gy));
        hipLaunchKernelGGL(select_samples_kernel, dim3(gx, gy), dim3(256), 0, stream, src->planes, idx, dst->planes, src->n_pad, dst->n_pad,
                           (unsigned)dst->n, (unsigned)(y0 * 64), (unsigned)src->groups);
    }
}

// the file rules' bitmap as the kernels read it: four 32-site words per group, zero behind the last column
static int upload_keep_words(const tracs_alignment *a, const uint64_t *keep, DeviceArray<uint4> &out, hipStream_t stream)
{
    if (const int rc = out.alloc(a->groups, "sample rule bitmap")) return rc;
    TRACS_HIP_CHECK(hipMemsetAsync(out.get(), 0, a->groups * 16, stream));
    TRACS_HIP_CHECK(hipMemcpyAsync(out.get(), keep, (a->L + 63) / 64 * 8, hipMemcpyHostToDevice, stream));
    return TRACS_OK;
}

// per sample, its N sites among the columns `keep` leaves (include/tracs_hip.h: tracs_alignment_sample_n_counts)
int sample_n_counts(const tracs_alignment *a, const uint64_t *keep, size_t keep_len, uint32_t *counts, hipStream_t stream)
{
    if (!a || (!counts && a->n)) { set_error("tracs_alignment_sample_n_counts: NULL argument"); return TRACS_E_ARG; }
    if (keep && keep_len != a->L) {
        set_error("sample rule: the keep bitmap covers " + std::to_string(keep_len) + " sites, the alignment has " + std::to_string(a->L));
        return TRACS_E_ARG;
    }
    if (!a->n) return TRACS_OK;
    DeviceCall guard(stream);
    TRACS_HIP_CHECK(hipMemsetAsync(counts, 0, a->n * 4, stream));
    if (!a->L) return TRACS_OK;
    DeviceArray<uint4> keepw;
    if (keep) {
        const int rc = upload_keep_words(a, keep, keepw, stream);
        if (rc) return rc;
    }
    launch_sample_counts(a, keepw.get(), counts, stream);
    TRACS_HIP_CHECK(hipGetLastError());
    if (keep) TRACS_HIP_CHECK(hipStreamSynchronize(stream));           // (the bitmap is this call's own: it goes once the kernel has read it)
    return TRACS_OK;
}

// the kept samples of `src` gathered into a new handle (include/tracs_hip.h: tracs_alignment_select_samples).  release_src_arena: the
// caller frees `src` right afterwards (the FASTA entry points), so its arena -- nothing has been built in it yet -- goes before the new
// handle's planes and arena are allocated, as in select_sites: the peak is source planes + new planes + one arena.
int select_samples(tracs_alignment *src, const uint8_t *keep_sample, tracs_alignment **out, hipStream_t stream, bool release_src_arena)
{
    if (out) *out = nullptr;
    if (!src || !out || (!keep_sample && src->n)) { set_error("tracs_alignment_select_samples: NULL argument"); return TRACS_E_ARG; }
    std::vector<unsigned> idx;
    for (size_t s = 0; s < src->n; s++)
        if (keep_sample[s]) idx.push_back((unsigned)s);
    if (idx.empty()) { set_error("no sample left after the sample rule"); return TRACS_E_ARG; }
    DeviceCall guard(stream);
    if (release_src_arena && src->arena && src->arena_used == 0 && src->pack_extra.empty()) {
        device_free(src->arena);
        src->arena = nullptr;
        src->arena_bytes = 0;
    }
    tracs_alignment *made = nullptr;
    int rc = tracs_alignment_create(idx.size(), src->L, &made);
    if (rc) return rc;
    AlignmentOwner dst(made);
    if (src->L) {
        DeviceArray<unsigned> d_idx;
        if ((rc = d_idx.alloc(idx.size(), "kept samples"))) return rc;
        TRACS_HIP_CHECK(hipMemcpyAsync(d_idx.get(), idx.data(), idx.size() * 4, hipMemcpyHostToDevice, stream));
        TRACS_HIP_CHECK(hipStreamSynchronize(nullptr));           // the new planes are cleared on the null stream
        launch_select_samples(src, d_idx.get(), dst.get(), stream);
        TRACS_HIP_CHECK(hipGetLastError());
        TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    }
    *out = dst.release();
    return TRACS_OK;
}

// the veto pass on the library's own panels (capi.hip) and behind tracs_pairs_min_sites
int pairs_min_sites(uint32_t *dist, const uint32_t *ncomp, size_t ld, size_t n, size_t row_begin, size_t row_end, size_t col_begin,
                    int32_t dist_threshold, uint32_t min_sites, hipStream_t stream)
{
    if (!min_sites) return TRACS_OK;
    if (!dist || !ncomp) { set_error("tracs_pairs_min_sites: NULL argument"); return TRACS_E_ARG; }
    if (ld < n) { set_error("tracs_pairs_min_sites: ld < n"); return TRACS_E_ARG; }
    if (n >= (1ull << 31)) { set_error("tracs_pairs_min_sites: n must be below 2^31"); return TRACS_E_ARG; }
    if (row_end > n) row_end = n;
    if (row_end <= row_begin || dist_threshold < 0 || col_begin >= n) return TRACS_OK;     // no row, no column, or no cell within the threshold
    const size_t nrows = row_end - row_begin;
    const unsigned gx = (unsigned)std::min<size_t>((n + 255) / 256, 64);
    const unsigned gy = (unsigned)std::min<size_t>(nrows, std::max<size_t>(1, 4096 / gx));
    hipLaunchKernelGGL(pair_min_sites_kernel, dim3(gx, gy), dim3(256), 0, stream, dist, ncomp, ld, (unsigned)n, (unsigned)row_begin, (unsigned)row_end,
                       (unsigned)col_begin, (unsigned)dist_threshold, min_sites);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

}  // namespace tracs

using namespace tracs;

extern "C" {

int tracs_alignment_sample_n_counts(const tracs_alignment *a, const uint64_t *keep, size_t keep_len, uint32_t *counts, void *stream)
{
    return sample_n_counts(a, keep, keep_len, counts, static_cast<hipStream_t>(stream));
}

int tracs_alignment_select_samples(const tracs_alignment *src, const uint8_t *keep_sample, tracs_alignment **out, void *stream)
{
    return select_samples(const_cast<tracs_alignment *>(src), keep_sample, out, static_cast<hipStream_t>(stream), false);
}

int tracs_pairs_min_sites(uint32_t *dist, const uint32_t *ncomp, size_t ld, size_t n, size_t row_begin, size_t row_end, size_t col_begin,
                          int32_t dist_threshold, uint32_t min_sites, void *stream)
{
    return pairs_min_sites(dist, ncomp, ld, n, row_begin, row_end, col_begin, dist_threshold, min_sites, static_cast<hipStream_t>(stream));
}

// Measurement (scripts/bench_samples.py): the count kernel (under `keep` where given) and the gather of the samples `keep_sample`
// keeps, between HIP events, `repeats` times after one warm-up round.  ms: [repeats][2] = count, gather.  The gathered handle is freed.
int tracs_debug_sample_select_timing(const tracs_alignment *src, const uint64_t *keep, size_t keep_len, const uint8_t *keep_sample, int repeats,
                                     float *ms, size_t *n_kept)
{
    if (!src || !keep_sample || !ms || repeats < 1 || !src->n || !src->L) { set_error("tracs_debug_sample_select_timing: bad argument"); return TRACS_E_ARG; }
    if (keep && keep_len != src->L) { set_error("tracs_debug_sample_select_timing: the keep bitmap does not cover the alignment"); return TRACS_E_ARG; }
    std::vector<unsigned> idx;
    for (size_t s = 0; s < src->n; s++)
        if (keep_sample[s]) idx.push_back((unsigned)s);
    if (idx.empty()) { set_error("no sample left after the sample rule"); return TRACS_E_ARG; }
    hipStream_t stream = nullptr;
    DeviceCall guard(stream);
    OwnedEvents<3> ev;
    DeviceArray<unsigned> d_idx, d_counts;
    DeviceArray<uint4> keepw;
    int rc = ev.create();
    if (rc || (keep && (rc = upload_keep_words(src, keep, keepw, stream)))) return rc;
    if ((rc = d_counts.alloc(src->n, "sample counts")) || (rc = d_idx.alloc(idx.size(), "kept samples"))) return rc;
    TRACS_HIP_CHECK(hipMemcpy(d_idx.get(), idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    tracs_alignment *made = nullptr;
    if ((rc = tracs_alignment_create(idx.size(), src->L, &made))) return rc;
    AlignmentOwner dst(made);
    TRACS_HIP_CHECK(hipDeviceSynchronize());
    for (int r = -1; r < repeats; r++) {                    // r = -1: warm-up
        TRACS_HIP_CHECK(hipMemsetAsync(d_counts.get(), 0, src->n * 4, stream));
        TRACS_HIP_CHECK(hipEventRecord(ev[0], stream));
        launch_sample_counts(src, keepw.get(), d_counts.get(), stream);
        TRACS_HIP_CHECK(hipEventRecord(ev[1], stream));
        launch_select_samples(src, d_idx.get(), dst.get(), stream);
        TRACS_HIP_CHECK(hipEventRecord(ev[2], stream));
        TRACS_HIP_CHECK(hipGetLastError());
        TRACS_HIP_CHECK(hipEventSynchronize(ev[2]));
        if (r >= 0)
            for (int k = 0; k < 2; k++) TRACS_HIP_CHECK(hipEventElapsedTime(&ms[r * 2 + k], ev[k], ev[k + 1]));
    }
    if (n_kept) *n_kept = idx.size();
    return TRACS_OK;
}

}  // extern "C"
