// tree_mask.hip -- verdicts on (branch, site) turned back into an alignment (gfx950).  Not in the reference.
//
// tracs_alignment_mask_subtrees sets the cell (i, s) of a packed alignment to N for every dropped entry (edge e, site s) of the branch
// filter's lists and every sample i below e -- the leaves in the subtree of e's child, the side away from the tree's top node.
//
//     host                 the tree is checked as tracs_fitch_count checks it and the edges' offsets as tracs_filter_recomb_lists checks
//                          them, before anything is launched.  One pass up the edges gives every node's number of leaves, one pass down
//                          a leaf order (a depth-first walk from the top node) in which the leaves below edge e are the interval
//                          [lo_e, lo_e + size_e).  O(n).
//     mask_weights_kernel  one lane per entry: its edge by binary search in edge_off (as flt_lists_kernel finds its list), its weight
//                          (size_e if dropped, else 0) and lo_e.
//     offsets_scan_launch  the weights into offsets; the total W is the number of (entry, leaf) cells, 64-bit.
//     mask_cells_kernel    one lane per cell of a range of W: the entry by binary search in the scanned weights, the leaf from the
//                          order, then the site's bit ORed into the 32-bit words of the five planes.  The OR is atomic, because the
//                          entries of several edges and sites share a word; a cell whose N bit is already set is left alone (bits are
//                          never cleared, so a set bit read without an atomic is final).  The lanes that set an N bit that was clear are
//                          counted per wave, and one lane adds the wave's count to a 64-bit sum: a set property, so deterministic.
//
// Nothing is stored for an entry with site >= L or a leaf >= n, so tail bits and pad samples stay zero.  Masking counts as a re-pack.
#include "common.h"
#include "scan_kernels.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

namespace tracs {

namespace {

constexpr unsigned long long MASK_RANGE = 1ull << 30;      // cells per launch: 2^22 workgroups of 256

// TRACS_MASK_RANGE (diagnostic; tests): cells per launch instead, at most MASK_RANGE, so that small inputs cross ranges.  Read per call.
unsigned long long mask_range()
{
    const unsigned long long v = sw::size(sw::TRACS_MASK_RANGE, 0);
    return v >= 1 && v <= MASK_RANGE ? v : MASK_RANGE;
}

__global__ __launch_bounds__(256) void mask_weights_kernel(const long long *__restrict__ edge_off, size_t n_edges, size_t total,
                                                           const uint8_t *__restrict__ dropped, const unsigned *__restrict__ edge_lo,
                                                           const unsigned *__restrict__ edge_size, unsigned *__restrict__ weight,
                                                           unsigned *__restrict__ lo_out)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= total) return;
    size_t lo = 0, hi = n_edges;                                           // the last e in [0, n_edges) with edge_off[e] <= k
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) >> 1;
        if (edge_off[mid] <= (long long)k) lo = mid; else hi = mid;
    }
    weight[k] = dropped[k] ? edge_size[lo] : 0u;
    lo_out[k] = edge_lo[lo];
}

__global__ __launch_bounds__(256) void mask_cells_kernel(unsigned *__restrict__ planes, size_t n_pad, unsigned n, unsigned L,
                                                         const long long *__restrict__ off, size_t total, unsigned long long w0,
                                                         unsigned long long w1, const unsigned *__restrict__ edge_site,
                                                         const unsigned *__restrict__ entry_lo, const unsigned *__restrict__ order,
                                                         unsigned long long *__restrict__ n_cells)
{
    const unsigned long long c = w0 + (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    bool fresh = false;
    if (c < w1) {
        size_t lo = 0, hi = total;                                         // the last k in [0, total) with off[k] <= c: its weight is not 0
        while (hi - lo > 1) {
            const size_t mid = (lo + hi) >> 1;
            if ((unsigned long long)off[mid] <= c) lo = mid; else hi = mid;
        }
        const unsigned long long at = (unsigned long long)entry_lo[lo] + (c - (unsigned long long)off[lo]);
        const unsigned site = edge_site[lo];
        if (at < n && site < L) {
            const unsigned leaf = order[at];
            if (leaf < n) {
                const size_t g = site >> 7;
                const unsigned word = (site >> 5) & 3u, bit = 1u << (site & 31u);
                unsigned *const w = planes + ((g * NPLANES) * n_pad + leaf) * 4 + word;
                const size_t plane = n_pad * 4;
                if (!(__atomic_load_n(w + 4 * plane, __ATOMIC_RELAXED) & bit)) {
                    for (int p = 0; p < 4; p++) atomicOr(w + p * plane, bit);
                    fresh = !(atomicOr(w + 4 * plane, bit) & bit);
                }
            }
        }
    }
    const unsigned long long set = __ballot(fresh);
    if ((threadIdx.x & 63u) == 0 && set) atomicAdd(n_cells, (unsigned long long)__popcll(set));
}

}  // namespace

int copy_planes(const char *who, tracs_alignment *dst, const tracs_alignment *src, hipStream_t stream)
{
    if (!dst || !src || dst == src || dst->n != src->n || dst->L != src->L || dst->n_pad != src->n_pad || dst->groups != src->groups) {
        set_error(std::string(who) + ": two distinct handles of one shape are needed");
        return TRACS_E_ARG;
    }
    DeviceCall guard(stream);
    dst->dirty = true;                                                     // packed again: every cached derived form goes
    dst->flt_stale = true;
    const size_t bytes = tracs_alignment_bytes(src);
    if (bytes) TRACS_HIP_CHECK(hipMemcpyAsync(dst->planes, src->planes, bytes, hipMemcpyDeviceToDevice, stream));
    return TRACS_OK;
}

}  // namespace tracs

using namespace tracs;

extern "C" {

int tracs_alignment_clone(const tracs_alignment *src, tracs_alignment **out, void *stream)
{
    if (out) *out = nullptr;
    if (!src || !out) { set_error("tracs_alignment_clone: NULL argument"); return TRACS_E_ARG; }
    tracs_alignment *a = nullptr;
    const int rc = tracs_alignment_create(src->n, src->L, &a);
    if (rc == TRACS_E_NOMEM) {
        (void)hipGetLastError();
        set_error("tracs_alignment_clone: a second copy of the alignment (" + std::to_string(tracs_alignment_bytes(src)) +
                  " bytes) does not fit in the device's memory");
    }
    if (rc) return rc;
    const int rc_copy = copy_planes("tracs_alignment_clone", a, src, static_cast<hipStream_t>(stream));
    if (rc_copy) { tracs_alignment_free(a); return rc_copy; }
    *out = a;
    return TRACS_OK;
}

int tracs_alignment_restore(tracs_alignment *dst, const tracs_alignment *src, void *stream)
{
    return copy_planes("tracs_alignment_restore", dst, src, static_cast<hipStream_t>(stream));
}

int tracs_alignment_mask_subtrees(tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, const int64_t *edge_off,
                                  const uint32_t *edge_site, const uint8_t *dropped, size_t n_entries, uint64_t *n_cells, void *stream)
{
    return mask_subtrees(a, parent, child, n_edges, edge_off, edge_site, dropped, n_entries, n_cells, nullptr, static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace tracs {

int mask_subtrees(tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, const int64_t *edge_off,
                  const uint32_t *edge_site, const uint8_t *dropped, size_t n_entries, uint64_t *n_cells, uint64_t *work, hipStream_t stream)
{
    static const char *const who = "tracs_alignment_mask_subtrees";
    if (n_cells) *n_cells = 0;
    if (work) *work = 0;
    if (!a) { set_error(std::string(who) + ": NULL alignment"); return TRACS_E_ARG; }
    if (a->L >= (1ull << 31)) { set_error(std::string(who) + ": alignment longer than 2^31 sites"); return TRACS_E_ARG; }
    int rc = nj_tree_check(who, a->n, parent, child, n_edges);
    if (rc) return rc;
    if (n_entries >= (1ull << 31)) { set_error(std::string(who) + ": more than 2^31 entries per call"); return TRACS_E_ARG; }
    if (!n_edges || !n_entries) return TRACS_OK;
    if (!edge_off || !edge_site || !dropped) { set_error(std::string(who) + ": NULL argument"); return TRACS_E_ARG; }
    DeviceCall guard(stream);
    // the offsets are checked on the host before anything is launched
    std::vector<long long> h_off(n_edges + 1);
    TRACS_HIP_CHECK(hipMemcpyAsync(h_off.data(), edge_off, (n_edges + 1) * 8, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    if (h_off[0] != 0) { set_error(std::string(who) + ": edge_off[0] must be 0"); return TRACS_E_ARG; }
    for (size_t e = 0; e < n_edges; e++)
        if (h_off[e + 1] < h_off[e]) { set_error(std::string(who) + ": the offsets decrease at edge " + std::to_string(e)); return TRACS_E_ARG; }
    if ((unsigned long long)h_off[n_edges] > n_entries) {
        set_error(std::string(who) + ": the offsets end at " + std::to_string(h_off[n_edges]) + ", beyond the " + std::to_string(n_entries) +
                  " entries given");
        return TRACS_E_ARG;
    }
    const size_t total = (size_t)h_off[n_edges];
    if (!total || !a->L || !a->planes) return TRACS_OK;
    // every node's leaves (children are older than their parents: one pass up), then the intervals (one pass down: a child's interval
    // starts where its parent's cursor stands).  n = 2: the edge (0, 1), whose lower side is the leaf 1.
    const size_t n = a->n, nodes = n >= 3 ? 2 * n - 2 : n;
    std::vector<uint32_t> size(nodes, 0), start(nodes, 0), cursor(nodes, 0), table(n + 2 * n_edges);
    uint32_t *const order = table.data(), *const edge_lo = order + n, *const edge_size = edge_lo + n_edges;
    for (size_t i = 0; i < n; i++) size[i] = 1;
    if (n == 2) {
        order[0] = 1; order[1] = 0;
        edge_lo[0] = 0; edge_size[0] = 1;
    } else {
        for (size_t e = 0; e < n_edges; e++) size[parent[e]] += size[child[e]];
        for (size_t e = n_edges; e-- > 0;) {
            const uint32_t p = parent[e], c = child[e];
            start[c] = cursor[c] = cursor[p];
            cursor[p] += size[c];
            edge_lo[e] = start[c]; edge_size[e] = size[c];
        }
        for (size_t i = 0; i < n; i++) order[start[i]] = (uint32_t)i;
    }
    unsigned *d_table, *d_weight, *d_lo;
    long long *d_off;
    unsigned long long *d_sums, *d_cells;
    if ((rc = workspace_get(WS_MASK_TREE, table.size(), &d_table)) || (rc = workspace_get(WS_MASK_WEIGHT, total, &d_weight)) ||
        (rc = workspace_get(WS_MASK_LO, total, &d_lo)) || (rc = workspace_get(WS_MASK_OFF, total + 1, &d_off)) ||
        (rc = workspace_get(WS_MASK_SUMS, offsets_scan_sums(total), &d_sums)) || (rc = workspace_get(WS_MASK_CELLS, 1, &d_cells))) return rc;
    TRACS_HIP_CHECK(hipMemcpyAsync(d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice, stream));
    TRACS_HIP_CHECK(hipMemsetAsync(d_cells, 0, 8, stream));
    hipLaunchKernelGGL(mask_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<const long long *>(edge_off),
                       n_edges, total, dropped, d_table + n, d_table + n + n_edges, d_weight, d_lo);
    if ((rc = offsets_scan_launch(d_weight, total, d_sums, d_off, stream))) return rc;
    long long W = 0;
    TRACS_HIP_CHECK(hipMemcpyAsync(&W, d_off + total, 8, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));                         // (also: the table is this call's memory)
    if (W > 0) {
        a->dirty = true;                                                   // packed again: every cached derived form goes
        a->flt_stale = true;
        const unsigned long long range = mask_range();
        for (unsigned long long w0 = 0; w0 < (unsigned long long)W; w0 += range) {
            const unsigned long long w1 = std::min<unsigned long long>((unsigned long long)W, w0 + range);
            hipLaunchKernelGGL(mask_cells_kernel, dim3((unsigned)((w1 - w0 + 255) / 256)), dim3(256), 0, stream,
                               reinterpret_cast<unsigned *>(a->planes), a->n_pad, (unsigned)n, (unsigned)a->L, d_off, total, w0, w1, edge_site, d_lo,
                               d_table, d_cells);
        }
        TRACS_HIP_CHECK(hipGetLastError());
        unsigned long long cells = 0;
        TRACS_HIP_CHECK(hipMemcpyAsync(&cells, d_cells, 8, hipMemcpyDeviceToHost, stream));
        TRACS_HIP_CHECK(hipStreamSynchronize(stream));
        if (n_cells) *n_cells = cells;
    }
    if (work) *work = (uint64_t)W;
    return TRACS_OK;
}

}  // namespace tracs
