// pair_sites.hip -- the SNP sites of listed pairs, with both alleles and the recombination filter's verdict per SNP (gfx950;
// DESIGN.md 3.15).
//
// Reference behaviour restated (never copied): /root/reference/src/pairsnp.hpp
//   the pair loop :398-403 (a site adds 1 to d(i, j) when (A_i & A_j) | (C_i & C_j) | (G_i & G_j) | (T_i & T_j) == 0),
//   filter_recomb :251-318 (which of those SNPs survive), range_count :223-248, cached_binomial_cdf :41-58.
// `tracs distance` reduces both to one count per pair; this file keeps the sites.  For m listed pairs (rows[t], cols[t]):
//
//     count    d[t] = the pair's SNP sites, from the four allele planes alone (no distance is supplied)
//     offsets  off = the exclusive scan of d (scan_kernels.h)
//     fill     the entries of pair t at [off[t], off[t + 1]), in site order: site[e] = the site (index into the packed alignment),
//              info[e] = the row sample's allele mask in bits 0-3 and the column sample's in bits 4-7 (A = 1, C = 2, G = 4, T = 8)
//     verdict  (filter) bit 8 of info[e] is set when filter_recomb drops that SNP: per SNP what filter.hip's filter_test_kernel
//              sums per pair -- filter_window, two binary searches for the window's count and span, filter_keep on the lgamma table
//
// Count and fill read like filter.hip's two extraction kernels, for the same reason (group-major, sample-minor planes: one pair
// reads isolated 16-byte segments): a wave per pair for short lists, a pair per lane for long row-major lists, where the 64 pairs
// of a wave mostly share their row and have consecutive columns.  A pass reads 8 plane rows x L / 8 bytes per pair; the fill adds
// 8 bytes per SNP.  Only the L real bits of the last word and the last group count.  Every store is bounded by the pair's own
// [off[t], off[t + 1]) AND by the capacity of the entry buffers, whatever the offsets hold.
#include "common.h"
#include "filter_math.h"
#include "scan_kernels.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

namespace tracs {

// bit b of the four allele planes' words -> the 4-bit mask
__device__ __forceinline__ unsigned ps_mask(unsigned a, unsigned c, unsigned g, unsigned t, int b)
{
    return ((a >> b) & 1u) | (((c >> b) & 1u) << 1) | (((g >> b) & 1u) << 2) | (((t >> b) & 1u) << 3);
}

// A wave per pair: lane l holds word base + l of both samples' four planes.  FILL = false: d[t] = the SNP bits; FILL = true: the
// entries, placed by an exclusive prefix of the lanes' popcounts (site order by construction).
template <bool FILL>
__global__ __launch_bounds__(64) void pair_sites_wave_kernel(const uint4 *__restrict__ P, size_t n, size_t n_pad, unsigned L,
                                                             const unsigned *__restrict__ rows, const unsigned *__restrict__ cols,
                                                             size_t n_pairs, const long long *__restrict__ off, long long base, long long room,
                                                             unsigned *__restrict__ site, unsigned *__restrict__ info,
                                                             unsigned *__restrict__ d, unsigned *__restrict__ bad)
{
    const int lane = threadIdx.x;
    const unsigned W = (L + 31) / 32;
    const size_t ps = n_pad * 4;                                           // plane stride in dwords
    for (size_t t = blockIdx.x; t < n_pairs; t += gridDim.x) {
        const size_t si = rows[t], sj = cols[t];
        if (si >= n || sj >= n) {                                          // (wave-uniform) never read outside the alignment
            if (lane == 0) { if (!FILL) d[t] = 0; if (bad) atomicOr(bad, 1u); }
            continue;
        }
        long long o = FILL ? off[t] - base : 0;
        const long long cap = FILL ? min(off[t + 1] - base, room) : 0;
        unsigned total = 0;
        for (unsigned w0 = 0; w0 < W; w0 += 64) {
            const unsigned w = w0 + lane;
            unsigned snp = 0, a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
            if (w < W) {
                const size_t g = w >> 2;
                const unsigned comp = w & 3;
                const unsigned *pi = reinterpret_cast<const unsigned *>(P + g * NPLANES * n_pad + si) + comp;
                const unsigned *pj = reinterpret_cast<const unsigned *>(P + g * NPLANES * n_pad + sj) + comp;
#pragma unroll
                for (int p = 0; p < 4; p++) { a[p] = pi[p * ps]; b[p] = pj[p * ps]; }
                snp = ~((a[0] & b[0]) | (a[1] & b[1]) | (a[2] & b[2]) | (a[3] & b[3]));      // :398-403
                const unsigned rem = L - w * 32;                           // only the L real bits
                if (rem < 32) snp &= (1u << rem) - 1u;
            }
            if (!FILL) { total += __popc(snp); continue; }
            unsigned c = __popc(snp), incl = c;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const unsigned v = __shfl_up(incl, s, 64);
                if (lane >= s) incl += v;
            }
            long long dst = o + (incl - c);
            while (snp) {
                const int bit = __ffs(snp) - 1;
                snp &= snp - 1;
                if (dst >= 0 && dst < cap) {
                    site[dst] = w * 32 + bit;
                    info[dst] = ps_mask(a[0], a[1], a[2], a[3], bit) | (ps_mask(b[0], b[1], b[2], b[3], bit) << 4);
                }
                dst++;
            }
            o += __shfl(incl, 63, 64);
        }
        if (!FILL) {
            for (int s = 32; s > 0; s >>= 1) total += __shfl_down(total, s, 64);
            if (lane == 0) d[t] = total;
        }
    }
}

// A pair per lane, every lane walks all groups: for long row-major lists the 64 pairs of a wave mostly share their row (one
// broadcast 16-byte load per plane) and have consecutive columns (64 x 16 bytes contiguous).
template <bool FILL>
__global__ __launch_bounds__(256) void pair_sites_lanes_kernel(const uint4 *__restrict__ P, size_t n, size_t n_pad, unsigned L, unsigned groups,
                                                               const unsigned *__restrict__ rows, const unsigned *__restrict__ cols,
                                                               size_t n_pairs, const long long *__restrict__ off, long long base, long long room,
                                                               unsigned *__restrict__ site, unsigned *__restrict__ info,
                                                               unsigned *__restrict__ d, unsigned *__restrict__ bad)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_pairs) return;
    const size_t si = rows[t], sj = cols[t];
    if (si >= n || sj >= n) {
        if (!FILL) d[t] = 0;
        if (bad) atomicOr(bad, 1u);
        return;
    }
    long long o = FILL ? off[t] - base : 0;
    const long long cap = FILL ? min(off[t + 1] - base, room) : 0;
    unsigned total = 0;
#pragma unroll 2
    for (unsigned g = 0; g < groups; g++) {
        const uint4 *pg = P + (size_t)g * NPLANES * n_pad;
        const uint4 a0 = pg[si], a1 = pg[n_pad + si], a2 = pg[2 * n_pad + si], a3 = pg[3 * n_pad + si];
        const uint4 b0 = pg[sj], b1 = pg[n_pad + sj], b2 = pg[2 * n_pad + sj], b3 = pg[3 * n_pad + sj];
        unsigned snp[4];                                                   // :398-403
        snp[0] = ~((a0.x & b0.x) | (a1.x & b1.x) | (a2.x & b2.x) | (a3.x & b3.x));
        snp[1] = ~((a0.y & b0.y) | (a1.y & b1.y) | (a2.y & b2.y) | (a3.y & b3.y));
        snp[2] = ~((a0.z & b0.z) | (a1.z & b1.z) | (a2.z & b2.z) | (a3.z & b3.z));
        snp[3] = ~((a0.w & b0.w) | (a1.w & b1.w) | (a2.w & b2.w) | (a3.w & b3.w));
        if (g + 1 == groups) {                                             // only the L real bits
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const unsigned long long first = ((unsigned long long)g * 4 + c) * 32;
                if (first >= L) snp[c] = 0;
                else if (L - first < 32) snp[c] &= (1u << (unsigned)(L - first)) - 1u;
            }
        }
        if (!FILL) { total += __popc(snp[0]) + __popc(snp[1]) + __popc(snp[2]) + __popc(snp[3]); continue; }
        if (!(snp[0] | snp[1] | snp[2] | snp[3])) continue;
        const unsigned aw[4][4] = {{a0.x, a1.x, a2.x, a3.x}, {a0.y, a1.y, a2.y, a3.y}, {a0.z, a1.z, a2.z, a3.z}, {a0.w, a1.w, a2.w, a3.w}};
        const unsigned bw[4][4] = {{b0.x, b1.x, b2.x, b3.x}, {b0.y, b1.y, b2.y, b3.y}, {b0.z, b1.z, b2.z, b3.z}, {b0.w, b1.w, b2.w, b3.w}};
#pragma unroll
        for (int c = 0; c < 4; c++) {
            unsigned s = snp[c];
            while (s) {
                const int bit = __ffs(s) - 1;
                s &= s - 1;
                if (o >= 0 && o < cap) {
                    site[o] = (g * 4 + c) * 32 + bit;
                    info[o] = ps_mask(aw[c][0], aw[c][1], aw[c][2], aw[c][3], bit) | (ps_mask(bw[c][0], bw[c][1], bw[c][2], bw[c][3], bit) << 4);
                }
                o++;
            }
        }
    }
    if (!FILL) d[t] = total;
}

__device__ __forceinline__ long long ps_lower_bound(const unsigned *a, long long n, long long key)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The filter's decision for every SNP of every pair (a wave per pair, lanes stride over its SNPs): filter_test_kernel's loop, with
// the decision stored instead of summed.  With d <= 1 every SNP is kept (:259-261); otherwise a SNP is kept when its window holds
// at most one SNP (:311) or 1 - CDF >= 0.05 / d (:294-309).
__global__ __launch_bounds__(64) void pair_sites_verdict_kernel(const unsigned *__restrict__ site, unsigned *__restrict__ info,
                                                                const long long *__restrict__ off, long long base, long long room,
                                                                size_t n_pairs, unsigned L, const double *__restrict__ lg)
{
    const int lane = threadIdx.x;
    for (size_t t = blockIdx.x; t < n_pairs; t += gridDim.x) {
        const long long o0 = off[t] - base, o1 = off[t + 1] - base;
        if (o0 < 0 || o1 < o0 || o1 > room) continue;
        const long long dn = o1 - o0;
        if (dn <= 1) continue;
        const unsigned *pos = site + o0;
        const FilterWindow fw = filter_window(dn, L);                      // :265-271
        for (long long u = lane; u < dn; u += 64) {
            const int i = (int)pos[u];
            const long long left = max(0, i - fw.wh);                      // :284
            const long long right = min((long long)(int)L, (long long)i + fw.wh + 1);      // :285
            const long long first = ps_lower_bound(pos, dn, left);
            const long long last = ps_lower_bound(pos, dn, right) - 1;
            const long long count = last - first + 1;
            if (count > 1) {
                const long long length = (long long)pos[last] - (long long)pos[first] + 1;   // :242
                if (!filter_keep(length, count, fw.p, fw.thr, lg)) info[o0 + u] |= 0x100u;
            }
        }
    }
}

int get_lgamma_table_for_filter(hipStream_t stream, const double **out);   // transcluster.hip


static size_t pair_sites_lanes_min()
{
    // a pair per lane needs enough pairs to fill the chip (every lane walks all groups); below that, a wave per pair
    return (size_t)sw::size(sw::TRACS_PAIR_SITES_LANES_MIN, 16384);
}

static int pair_sites_check(const tracs_alignment *a, const char *who)
{
    if (!a || !a->planes) { set_error(std::string(who) + ": NULL alignment"); return TRACS_E_ARG; }
    if (a->L >= (1ull << 31)) { set_error(std::string(who) + ": alignment longer than 2^31 sites"); return TRACS_E_ARG; }
    return TRACS_OK;
}

// d[0 .. n_pairs) and off[0 .. n_pairs] (device); *total (host) = off[n_pairs].  Synchronises the stream.
int pair_sites_count(const tracs_alignment *a, const unsigned *rows, const unsigned *cols, size_t n_pairs, unsigned *d, long long *off,
                     uint64_t *total, hipStream_t stream)
{
    if (total) *total = 0;
    int rc = pair_sites_check(a, "tracs_pair_sites_count");
    if (rc) return rc;
    if (!off || (n_pairs && (!rows || !cols || !d))) { set_error("tracs_pair_sites_count: NULL argument"); return TRACS_E_ARG; }
    DeviceCall guard(stream);
    unsigned long long *sums;
    unsigned *bad;
    if ((rc = workspace_get(WS_PSITES_SUMS, offsets_scan_sums(n_pairs), &sums)) ||
        (rc = workspace_get(WS_PSITES_BAD, 16, &bad))) return rc;
    TRACS_HIP_CHECK(hipMemsetAsync(bad, 0, 4, stream));
    if (n_pairs) {
        if (n_pairs >= pair_sites_lanes_min())
            hipLaunchKernelGGL(pair_sites_lanes_kernel<false>, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, stream, a->planes, a->n,
                               a->n_pad, (unsigned)a->L, (unsigned)a->groups, rows, cols, n_pairs, nullptr, 0ll, 0ll, nullptr, nullptr, d, bad);
        else
            hipLaunchKernelGGL(pair_sites_wave_kernel<false>, dim3((unsigned)std::min<size_t>(n_pairs, 256 * 64)), dim3(64), 0, stream, a->planes,
                               a->n, a->n_pad, (unsigned)a->L, rows, cols, n_pairs, nullptr, 0ll, 0ll, nullptr, nullptr, d, bad);
        TRACS_HIP_CHECK(hipGetLastError());
    }
    if ((rc = offsets_scan_launch(d, n_pairs, sums, off, stream))) return rc;
    long long tot = 0;
    unsigned flag = 0;
    TRACS_HIP_CHECK(hipMemcpyAsync(&tot, off + n_pairs, 8, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipMemcpyAsync(&flag, bad, 4, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    if (flag) { set_error("tracs_pair_sites_count: a listed sample index is outside the alignment"); return TRACS_E_ARG; }
    if (total) *total = (uint64_t)tot;
    return TRACS_OK;
}

// The entries of the pairs at site / info [off[t] - base, off[t + 1] - base) (room: entries the two buffers hold); filter: verdicts.
int pair_sites_fill(const tracs_alignment *a, const unsigned *rows, const unsigned *cols, size_t n_pairs, const long long *off, long long base,
                    unsigned *site, unsigned *info, size_t room, int filter, hipStream_t stream)
{
    int rc = pair_sites_check(a, "tracs_pair_sites_fill");
    if (rc) return rc;
    if (!n_pairs || !room) return TRACS_OK;
    if (!rows || !cols || !off || !site || !info) { set_error("tracs_pair_sites_fill: NULL argument"); return TRACS_E_ARG; }
    DeviceCall guard(stream);
    const double *lg = nullptr;
    if (filter && (rc = get_lgamma_table_for_filter(stream, &lg))) return rc;
    const unsigned blocks = (unsigned)std::min<size_t>(n_pairs, 256 * 64);
    if (n_pairs >= pair_sites_lanes_min())
        hipLaunchKernelGGL(pair_sites_lanes_kernel<true>, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, stream, a->planes, a->n, a->n_pad,
                           (unsigned)a->L, (unsigned)a->groups, rows, cols, n_pairs, off, base, (long long)room, site, info, nullptr, nullptr);
    else
        hipLaunchKernelGGL(pair_sites_wave_kernel<true>, dim3(blocks), dim3(64), 0, stream, a->planes, a->n, a->n_pad, (unsigned)a->L, rows, cols,
                           n_pairs, off, base, (long long)room, site, info, nullptr, nullptr);
    if (filter)
        hipLaunchKernelGGL(pair_sites_verdict_kernel, dim3(blocks), dim3(64), 0, stream, site, info, off, base, (long long)room, n_pairs,
                           (unsigned)a->L, lg);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

// ---- the rows of `tracs pair-sites` -------------------------------------------------------------------------------------------------
static inline void ps_append_u64(std::string &s, uint64_t v)
{
    char buf[24];
    int k = 24;
    do { buf[--k] = (char)('0' + v % 10); v /= 10; } while (v);
    s.append(buf + k, 24 - k);
}

// Count every pair, refuse before anything is written when the entries exceed max_entries, then fill batch by batch: device entry
// buffer -> pinned host buffer -> rows formatted on host threads and appended in order.  The two buffers hold at most 256 MiB each
// (TRACS_PAIR_SITES_BATCH: entries per batch instead, for tests), or one pair's entries when a pair has more -- whatever the list
// holds.  The steps of a batch run one after another on the null stream; the buffers bound memory, they do not pipeline.
// kept (may be NULL: every column): the kept-columns bitmap over the source_len columns read; contigs (may be none): names
// and lengths in file order, positions are then relative to the contig's first column.
int pair_sites_write(const tracs_alignment *a, const char *const *names, const uint64_t *kept, size_t source_len, const uint32_t *rows,
                     const uint32_t *cols, size_t n_pairs, int filter, uint64_t max_entries, const char *path, const char *const *contig_names,
                     const uint64_t *contig_lengths, size_t n_contigs, int n_threads, uint64_t *rows_written)
{
    if (rows_written) *rows_written = 0;
    int rc = pair_sites_check(a, "tracs_distance_pair_sites");
    if (rc) return rc;
    if (!path || !names || (n_pairs && (!rows || !cols)) || (n_contigs && (!contig_names || !contig_lengths))) {
        set_error("tracs_distance_pair_sites: NULL argument");
        return TRACS_E_ARG;
    }
    for (size_t t = 0; t < n_pairs; t++)
        if (rows[t] >= a->n || cols[t] >= a->n) { set_error("tracs_distance_pair_sites: pair " + std::to_string(t) + " names a sample outside the alignment"); return TRACS_E_ARG; }
    // kept column -> column of the files read
    std::vector<uint64_t> src_col;
    if (kept) {
        src_col.reserve(a->L);
        for (size_t s = 0; s < source_len; s++)
            if ((kept[s >> 6] >> (s & 63)) & 1ull) src_col.push_back(s);
        if (src_col.size() != a->L) { set_error("tracs_distance_pair_sites: the kept-columns bitmap does not match the alignment"); return TRACS_E_ARG; }
    }
    std::vector<uint64_t> contig_end(n_contigs);
    { uint64_t o = 0; for (size_t c = 0; c < n_contigs; c++) { o += contig_lengths[c]; contig_end[c] = o; } }
    if (n_contigs && a->L) {
        const uint64_t last = kept ? src_col.back() : a->L - 1;
        if (last >= contig_end.back()) {
            set_error("the alignment reaches column " + std::to_string(last) + ", past the reference's contigs (" + std::to_string(contig_end.back()) + ")");
            return TRACS_E_ARG;
        }
    }
    DeviceCall guard(nullptr);
    DeviceArray<unsigned> rows_buf, cols_buf, d_buf, ent_buf;
    PinnedArray<unsigned> host_buf;
    DeviceArray<long long> off_buf;
    const size_t np1 = std::max<size_t>(n_pairs, 1);
    if ((rc = rows_buf.alloc(np1, "pair rows")) || (rc = cols_buf.alloc(np1, "pair columns")) || (rc = d_buf.alloc(np1, "pair distances")) ||
        (rc = off_buf.alloc(n_pairs + 1, "pair offsets"))) return rc;
    unsigned *const d_rows = rows_buf.get(), *const d_cols = cols_buf.get(), *const d_d = d_buf.get();
    long long *const d_off = off_buf.get();
    if (n_pairs) {
        TRACS_HIP_CHECK(hipMemcpy(d_rows, rows, n_pairs * 4, hipMemcpyHostToDevice));
        TRACS_HIP_CHECK(hipMemcpy(d_cols, cols, n_pairs * 4, hipMemcpyHostToDevice));
    }
    uint64_t total = 0;
    if ((rc = pair_sites_count(a, d_rows, d_cols, n_pairs, d_d, d_off, &total, nullptr))) return rc;
    if (total > max_entries) {
        set_error("the listed pairs differ at " + std::to_string(total) + " sites in all, more than --max-entries " + std::to_string(max_entries) +
                  "; nothing was written");
        return TRACS_E_ARG;
    }
    std::vector<long long> off(n_pairs + 1, 0);
    TRACS_HIP_CHECK(hipMemcpy(off.data(), d_off, (n_pairs + 1) * 8, hipMemcpyDeviceToHost));
    const size_t cap = std::max<size_t>(1, (size_t)sw::size(sw::TRACS_PAIR_SITES_BATCH, (256ull << 20) / 8));     // entries per batch: 8 bytes each
    long long max_d = 0;
    for (size_t t = 0; t < n_pairs; t++) max_d = std::max(max_d, off[t + 1] - off[t]);
    const size_t room = std::max<size_t>(std::max<size_t>(std::min<size_t>(cap, total), (size_t)max_d), 1);
    if (total && ((rc = ent_buf.alloc(room * 2, "pair-site entries")) || (rc = host_buf.alloc(room * 2, "pair-site entries")))) return rc;
    unsigned *const d_ent = ent_buf.get(), *const h_ent = host_buf.get();
    std::unique_ptr<FILE, int (*)(FILE *)> file(std::fopen(path, "w"), std::fclose);
    FILE *const fp = file.get();
    if (!fp) { set_error(std::string("cannot write ") + path); return TRACS_E_OPEN; }
    std::fputs("sampleA,sampleB,contig,position,alleleA,alleleB,dropped\n", fp);
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const size_t n_thr = n_threads > 0 ? std::min<size_t>((size_t)n_threads, 64) : hw;
    const size_t slice = 1u << 18;                                         // entries one thread formats at a time
    static const char letters[] = "XACMGRSVTWYHKDBN";
    std::vector<std::string> text(n_thr);
    for (size_t t0 = 0; t0 < n_pairs;) {
        size_t t1 = t0 + 1;                                                // (a batch is never less than one pair)
        while (t1 < n_pairs && (size_t)(off[t1 + 1] - off[t0]) <= cap) t1++;
        const long long base = off[t0];
        const size_t entries = (size_t)(off[t1] - base);
        if (entries) {
            if ((rc = pair_sites_fill(a, d_rows + t0, d_cols + t0, t1 - t0, d_off + t0, base, d_ent, d_ent + room, room, filter, nullptr))) return rc;
            TRACS_HIP_CHECK(hipMemcpy(h_ent, d_ent, entries * 4, hipMemcpyDeviceToHost));
            TRACS_HIP_CHECK(hipMemcpy(h_ent + room, d_ent + room, entries * 4, hipMemcpyDeviceToHost));
            const unsigned *h_site = h_ent, *h_info = h_ent + room;
            auto format = [&](size_t k, size_t e0, size_t e1) {
                std::string &s = text[k];
                s.clear();
                if (e0 >= e1) return;
                // the pair that holds entry e0: the last t with off[t] - base <= e0
                size_t t = (size_t)(std::upper_bound(off.begin() + t0, off.begin() + t1, base + (long long)e0) - off.begin()) - 1;
                std::string head;
                size_t head_of = (size_t)-1;
                for (size_t e = e0; e < e1; e++) {
                    while ((long long)e >= off[t + 1] - base) t++;
                    if (head_of != t) { head = std::string(names[rows[t]]) + "," + names[cols[t]] + ","; head_of = t; }
                    const uint64_t col = kept ? src_col[h_site[e]] : h_site[e];
                    s += head;
                    if (n_contigs) {
                        const size_t c = (size_t)(std::upper_bound(contig_end.begin(), contig_end.end(), col) - contig_end.begin());
                        s += contig_names[c];
                        s += ',';
                        ps_append_u64(s, col - (c ? contig_end[c - 1] : 0));
                    } else {
                        s += "alignment,";
                        ps_append_u64(s, col);
                    }
                    const unsigned v = h_info[e];
                    s += ',';
                    s += letters[v & 15u];
                    s += ',';
                    s += letters[(v >> 4) & 15u];
                    s += filter ? ((v & 0x100u) ? ",1\n" : ",0\n") : ",NA\n";
                }
            };
            for (size_t e0 = 0; e0 < entries; e0 += slice * n_thr) {
                const size_t e1 = std::min(entries, e0 + slice * n_thr);
                const size_t used = (e1 - e0 + slice - 1) / slice;
                if (used == 1) format(0, e0, e1);
                else {
                    std::vector<std::thread> pool;
                    for (size_t k = 0; k < used; k++) pool.emplace_back(format, k, e0 + k * slice, std::min(e1, e0 + (k + 1) * slice));
                    for (auto &th : pool) th.join();
                }
                for (size_t k = 0; k < used; k++)
                    if (!text[k].empty() && std::fwrite(text[k].data(), 1, text[k].size(), fp) != text[k].size()) {
                        set_error(std::string("write error on ") + path);
                        return TRACS_E_OPEN;
                    }
            }
        }
        t0 = t1;
    }
    if (std::fclose(file.release()) != 0) { set_error(std::string("write error on ") + path); return TRACS_E_OPEN; }
    if (rows_written) *rows_written = total;
    return TRACS_OK;
}

}  // namespace tracs

using namespace tracs;

extern "C" {

int tracs_pair_sites_count(const tracs_alignment *a, const uint32_t *rows, const uint32_t *cols, size_t n_pairs, uint32_t *d, int64_t *off,
                           uint64_t *total, void *stream)
{
    return pair_sites_count(a, rows, cols, n_pairs, d, reinterpret_cast<long long *>(off), total, static_cast<hipStream_t>(stream));
}

int tracs_pair_sites_fill(const tracs_alignment *a, const uint32_t *rows, const uint32_t *cols, size_t n_pairs, const int64_t *off,
                          int64_t entry_base, uint32_t *site, uint32_t *info, size_t room, int filter, void *stream)
{
    return pair_sites_fill(a, rows, cols, n_pairs, reinterpret_cast<const long long *>(off), (long long)entry_base, site, info, room, filter,
                           static_cast<hipStream_t>(stream));
}

}  // extern "C"
