// fitch.hip -- every site of the packed alignment placed on a fixed tree: small parsimony, Fitch's two passes (gfx950).
// Not in the reference.
//
// The tree is tracs_nj_edges's: join t = 0 .. n - 4 made node n + t from a_t < b_t, the top node 2n - 3 has x < y < z.  A sample's
// allele planes are its set per site (A = 1, C = 2, G = 4, T = 8; N = 15), and on 32 sites at a time Fitch's rule is an AND, a test for
// zero and an OR:
//
//     bottom-up   S_leaf = its mask; join: I = S_a & S_b, S = I if I != 0, else S_a | S_b; top: S_xy likewise, I = S_xy & S_z,
//                 S_T = I if I != 0, else S_xy
//     top-down    f_T = lowbit(S_T); edges by descending parent, creation order within a parent; f_child = f_parent if
//                 f_parent & S_child != 0, else lowbit(S_child); a change is an edge with f_child != f_parent
//     minimum     (the smallest |H| with m_i & H != 0 for every sample i) - 1, from 14 AND-accumulators of "some base of H present"
//
// One lane owns a word of 32 sites and walks the whole tree.  The sets of all 2n - 2 nodes for a SLAB of sites live in a workspace
// buffer laid out [node][word] (16 bytes per entry: the A, C, G, T words), so the lanes of a wave touch one contiguous run per node:
//
//     fitch_leaves_kernel   the slab's leaves out of the group-major, sample-minor planes into that layout through an LDS tile: read
//                           coalesced along samples (64 x 16 bytes per plane row), written coalesced along words (256 bytes per sample)
//     fitch_walk_kernel     both passes.  The top-down states overwrite the internal nodes' sets in place (a set is read once more, by
//                           the edge above it).  COUNT: the edges' sums (one atomicAdd of a wave's popcount: integer sums, no order
//                           depends on them), the sites' change counts from a bit-sliced counter (25 words per lane: one ripple add
//                           per edge with a change), the sites' minimum.  FILL: the same walk; the entries of site s go to
//                           off[s] - entry_base + (the site's counter so far), so they are in walk order without any atomic.
//                           ECOUNT / EFILL (tracs_fitch_edge_sites): the changes regrouped by edge.  A wave holds 2 048
//                           consecutive sites in lane order; ECOUNT stores the wave's popcount per edge into a [chunk][edge] matrix
//                           (one chunk per wave), fitch_edge_scan_kernel turns every column into bases (and carries a per-edge cursor
//                           from one range of chunks to the next), and EFILL walks again: a change goes to edge_off[e] +
//                           base[chunk][e] + (the popcounts of the lower lanes) + (its rank inside the word).  Ascending, no atomic.
//
// The slab is sized from a byte budget, not from n x L (TRACS_FITCH_SLAB_GROUPS forces its length in groups of 128 sites).  Only the L
// real bits of the last word count; pad samples are never read into the buffer; pad groups are never walked.  Every store of the
// fill is bounded by the site's own [off[s], off[s + 1]) AND by the capacity of the entry buffers, whatever the offsets hold.
#include "common.h"
#include "scan_kernels.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

namespace tracs {

namespace {

constexpr int FITCH_BITS = 25;                      // a site has at most 2n - 3 < 2^25 changes
constexpr size_t FITCH_MAX_N = (size_t)1 << 21;     // (the leaves kernel's grid: n / 64 workgroups in y)
constexpr size_t FITCH_SLAB_BYTES = 8ull << 30;     // the [node][word] buffer of one slab, at most
constexpr size_t FITCH_MATRIX_BYTES = 256ull << 20; // the [chunk][edge] matrix of one range of tracs_fitch_edge_sites, at most
constexpr unsigned FITCH_CHUNK_GROUPS = 16;         // a chunk is a wave of the walk: 64 words, 16 groups

// what a walk leaves behind
enum : int { FITCH_COUNT = 0, FITCH_FILL = 1, FITCH_ECOUNT = 2, FITCH_EFILL = 3 };

__device__ __forceinline__ uint4 fitch_join(const uint4 a, const uint4 b)
{
    const uint4 i = make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w);
    const unsigned z = ~(i.x | i.y | i.z | i.w);                            // sites with an empty intersection
    return make_uint4(i.x | ((a.x | b.x) & z), i.y | ((a.y | b.y) & z), i.z | ((a.z | b.z) & z), i.w | ((a.w | b.w) & z));
}

// the top node's third child: I = S_xy & S_z, else S_xy
__device__ __forceinline__ uint4 fitch_top(const uint4 xy, const uint4 c)
{
    const uint4 i = make_uint4(xy.x & c.x, xy.y & c.y, xy.z & c.z, xy.w & c.w);
    const unsigned z = ~(i.x | i.y | i.z | i.w);
    return make_uint4(i.x | (xy.x & z), i.y | (xy.y & z), i.z | (xy.z & z), i.w | (xy.w & z));
}

// lowbit per site: A before C before G before T
__device__ __forceinline__ uint4 fitch_low(const uint4 s)
{
    return make_uint4(s.x, s.y & ~s.x, s.z & ~(s.x | s.y), s.w & ~(s.x | s.y | s.z));
}

// f_child from f_parent (one-hot) and S_child; change <- the sites at which it is not f_parent
__device__ __forceinline__ uint4 fitch_child(const uint4 fp, const uint4 sc, unsigned &change)
{
    const unsigned hit = (fp.x & sc.x) | (fp.y & sc.y) | (fp.z & sc.z) | (fp.w & sc.w);
    const uint4 low = fitch_low(sc);
    change = ~hit;
    return make_uint4((fp.x & hit) | (low.x & ~hit), (fp.y & hit) | (low.y & ~hit), (fp.z & hit) | (low.z & ~hit), (fp.w & hit) | (low.w & ~hit));
}

__device__ __forceinline__ unsigned fitch_mask(const uint4 v, int b)
{
    return ((v.x >> b) & 1u) | (((v.y >> b) & 1u) << 1) | (((v.z >> b) & 1u) << 2) | (((v.w >> b) & 1u) << 3);
}

// the bit-sliced counters of a lane's 32 sites: c[k] holds bit k of every site's count
__device__ __forceinline__ void fitch_counter_add(unsigned (&c)[FITCH_BITS], unsigned x)
{
#pragma unroll
    for (int k = 0; k < FITCH_BITS; k++) { const unsigned t = c[k] & x; c[k] ^= x; x = t; }
}
__device__ __forceinline__ unsigned fitch_counter_get(const unsigned (&c)[FITCH_BITS], int b)
{
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < FITCH_BITS; k++) v |= ((c[k] >> b) & 1u) << k;
    return v;
}

// "some base of H is in every sample's mask so far", for the 14 proper subsets H: 4 of one base, 6 of two, 4 of three
__device__ __forceinline__ void fitch_min_add(unsigned (&m)[14], const uint4 s)
{
    m[0] &= s.x; m[1] &= s.y; m[2] &= s.z; m[3] &= s.w;
    m[4] &= s.x | s.y; m[5] &= s.x | s.z; m[6] &= s.x | s.w; m[7] &= s.y | s.z; m[8] &= s.y | s.w; m[9] &= s.z | s.w;
    m[10] &= s.x | s.y | s.z; m[11] &= s.x | s.y | s.w; m[12] &= s.x | s.z | s.w; m[13] &= s.y | s.z | s.w;
}

// The leaves of groups [g0, g0 + slab_groups) of samples [0, n) into buf[s * stride + (g - g0) * 4 + c] = (A, C, G, T word c).
// A workgroup takes 64 samples x 4 groups: thread (group, sample) reads its four plane entries (64 consecutive samples of one
// plane row per wave), the tile turns them, and 16 threads write one sample's 16 entries (256 contiguous bytes).
__global__ __launch_bounds__(256) void fitch_leaves_kernel(const uint4 *__restrict__ P, unsigned n, size_t n_pad, size_t g0, unsigned slab_groups,
                                                           uint4 *__restrict__ buf, size_t stride)
{
    __shared__ uint4 tile[64][17];                                         // (17: the rows of a wave's samples start in different banks)
    const unsigned tid = threadIdx.x, gi = tid >> 6, si = tid & 63;
    const unsigned gl = blockIdx.x * 4 + gi;
    const size_t s = (size_t)blockIdx.y * 64 + si;                         // < n_pad: a multiple of 64
    uint4 p[4];
#pragma unroll
    for (int q = 0; q < 4; q++) p[q] = make_uint4(0, 0, 0, 0);
    if (gl < slab_groups) {
        const uint4 *pg = P + (g0 + gl) * NPLANES * n_pad + s;
#pragma unroll
        for (int q = 0; q < 4; q++) p[q] = pg[(size_t)q * n_pad];
    }
    tile[si][gi * 4 + 0] = make_uint4(p[0].x, p[1].x, p[2].x, p[3].x);
    tile[si][gi * 4 + 1] = make_uint4(p[0].y, p[1].y, p[2].y, p[3].y);
    tile[si][gi * 4 + 2] = make_uint4(p[0].z, p[1].z, p[2].z, p[3].z);
    tile[si][gi * 4 + 3] = make_uint4(p[0].w, p[1].w, p[2].w, p[3].w);
    __syncthreads();
    const unsigned col = tid & 15;
    const unsigned wl = blockIdx.x * 16 + col;
    if (wl >= slab_groups * 4) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned row = (tid >> 4) + 16 * k;
        const size_t sample = (size_t)blockIdx.y * 64 + row;
        if (sample < n) buf[sample * stride + wl] = tile[row][col];
    }
}

// Both passes for the words [word0, word0 + n_words) of a slab (lane = word), sites [site_begin, site_end) only.  child: the edge
// list's child column (device); every lane reads the same entries.
// ECOUNT: edge_changes is the launch's part of the chunk matrix, [blockIdx.x][edge]; every (chunk, edge) is stored.  EFILL: edge_changes
// is that part after the scan (bases), off is edge_off, site is edge_site and room its capacity; base, edge, info are not used.
template <int MODE>
__global__ __launch_bounds__(64) void fitch_walk_kernel(uint4 *__restrict__ buf, size_t stride, unsigned n, const unsigned *__restrict__ child,
                                                        unsigned word0, unsigned n_words, unsigned site_begin, unsigned site_end,
                                                        unsigned *__restrict__ edge_changes, unsigned *__restrict__ site_changes,
                                                        uint8_t *__restrict__ site_minimum, const long long *__restrict__ off, long long base,
                                                        long long room, unsigned *__restrict__ site, unsigned *__restrict__ edge,
                                                        unsigned *__restrict__ info)
{
    const unsigned lane = threadIdx.x;
    const unsigned wl = blockIdx.x * 64 + lane;
    const bool active = wl < n_words;                                      // an inactive lane touches no memory and has no valid site
    const unsigned w = word0 + wl;
    unsigned valid = 0;
    if (active) {
        const unsigned long long first = (unsigned long long)w * 32;
        const unsigned long long lo = max(first, (unsigned long long)site_begin), hi = min(first + 32, (unsigned long long)site_end);
        if (hi > lo) valid = (hi - lo == 32 ? ~0u : ((1u << (unsigned)(hi - lo)) - 1u)) << (unsigned)(lo - first);
    }
    uint4 *col = buf + (active ? wl : 0);
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    unsigned cnt[FITCH_BITS];
#pragma unroll
    for (int k = 0; k < FITCH_BITS; k++) cnt[k] = 0;
    unsigned mn[14];
#pragma unroll
    for (int k = 0; k < 14; k++) mn[k] = ~0u;

    const size_t n_edges = n >= 3 ? 2 * (size_t)n - 3 : (size_t)n - 1;
    // one edge of the top-down walk: e, its changes among the valid sites, both states
    auto emit = [&](unsigned e, unsigned ch, const uint4 fp, const uint4 fc) {
        if (MODE == FITCH_ECOUNT) {
            unsigned c = 0;
            if (__ballot(ch != 0)) {                                       // (wave-uniform)
                c = __popc(ch);
                for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s, 64);
            }
            if (lane == 0) edge_changes[(size_t)blockIdx.x * n_edges + e] = c;
            return;
        }
        if (MODE == FITCH_EFILL) {
            if (!__ballot(ch != 0)) return;                                // (wave-uniform)
            const unsigned c = __popc(ch);
            unsigned incl = c;
            for (int o = 1; o < 64; o <<= 1) { const unsigned x = __shfl_up(incl, o, 64); if (lane >= (unsigned)o) incl += x; }
            if (ch) {
                long long dst = off[e] + (long long)edge_changes[(size_t)blockIdx.x * n_edges + e] + (long long)(incl - c);
                const long long cap = min(off[e + 1], room);
                unsigned r = ch;
                while (r) {
                    const int b = __ffs(r) - 1;
                    r &= r - 1;
                    if (dst >= 0 && dst < cap) site[dst] = w * 32 + (unsigned)b;
                    dst++;
                }
            }
            return;
        }
        if (MODE == FITCH_COUNT) {
            if (__ballot(ch != 0)) {                                       // (wave-uniform)
                unsigned c = __popc(ch);
                for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s, 64);
                if (lane == 0) atomicAdd(edge_changes + e, c);
            }
        } else {
            unsigned r = ch;
            while (r) {
                const int b = __ffs(r) - 1;
                r &= r - 1;
                const size_t s = (size_t)w * 32 + b;
                const long long dst = off[s] - base + (long long)fitch_counter_get(cnt, b);
                const long long cap = min(off[s + 1] - base, room);
                if (dst >= 0 && dst < cap) {
                    site[dst] = (unsigned)s;
                    edge[dst] = e;
                    info[dst] = fitch_mask(fp, b) | (fitch_mask(fc, b) << 4);
                }
            }
        }
        if (ch) fitch_counter_add(cnt, ch);
    };
    // the edge (parent state fp, child c): the child's state, kept in its slot when it is an internal node
    auto down = [&](unsigned e, unsigned c, const uint4 fp) {
        unsigned ch = 0;
        uint4 fc = zero4;
        if (active) {
            const uint4 sc = col[(size_t)c * stride];
            fc = fitch_child(fp, sc, ch);
            ch &= valid;
            if (c >= n) col[(size_t)c * stride] = fc;
        }
        emit(e, ch, fp, fc);
    };

    if (n == 1) {
        if (active && MODE == FITCH_COUNT) fitch_min_add(mn, col[0]);
    } else if (n == 2) {
        // the one edge (0, 1): f_0 = lowbit(m_0 & m_1), or lowbit(m_0) where that is empty
        uint4 f0 = zero4, f1 = zero4;
        unsigned ch = 0;
        if (active) {
            const uint4 m0 = col[0], m1 = col[stride];
            if (MODE == FITCH_COUNT) { fitch_min_add(mn, m0); fitch_min_add(mn, m1); }
            f0 = fitch_low(fitch_top(m0, m1));
            f1 = fitch_child(f0, m1, ch);
            ch &= valid;
        }
        emit(0, ch, f0, f1);
    } else {
        const unsigned J = n - 3, top = n + J;
        for (unsigned t = 0; t < J; t++) {
            const unsigned a = child[2 * t], b = child[2 * t + 1];
            if (active) {
                const uint4 sa = col[(size_t)a * stride], sb = col[(size_t)b * stride];
                if (MODE == FITCH_COUNT) {
                    if (a < n) fitch_min_add(mn, sa);
                    if (b < n) fitch_min_add(mn, sb);
                }
                col[(size_t)(n + t) * stride] = fitch_join(sa, sb);
            }
        }
        const unsigned x = child[2 * J], y = child[2 * J + 1], z = child[2 * J + 2];
        uint4 ft = zero4;
        if (active) {
            const uint4 sx = col[(size_t)x * stride], sy = col[(size_t)y * stride], sz = col[(size_t)z * stride];
            if (MODE == FITCH_COUNT) {
                if (x < n) fitch_min_add(mn, sx);
                if (y < n) fitch_min_add(mn, sy);
                if (z < n) fitch_min_add(mn, sz);
            }
            ft = fitch_low(fitch_top(fitch_join(sx, sy), sz));
            col[(size_t)top * stride] = ft;
        }
        down(2 * J, x, ft);
        down(2 * J + 1, y, ft);
        down(2 * J + 2, z, ft);
        for (unsigned t = J; t-- > 0;) {
            const unsigned a = child[2 * t], b = child[2 * t + 1];
            const uint4 fp = active ? col[(size_t)(n + t) * stride] : zero4;
            down(2 * t, a, fp);
            down(2 * t + 1, b, fp);
        }
    }
    if (MODE == FITCH_COUNT && valid) {
        const unsigned one = mn[0] | mn[1] | mn[2] | mn[3];
        const unsigned two = mn[4] | mn[5] | mn[6] | mn[7] | mn[8] | mn[9];
        const unsigned three = mn[10] | mn[11] | mn[12] | mn[13];
        for (int b = 0; b < 32; b++) {
            if (!((valid >> b) & 1u)) continue;
            const size_t s = (size_t)w * 32 + b;
            site_changes[s] = fitch_counter_get(cnt, b);
            site_minimum[s] = (uint8_t)(((one >> b) & 1u) ? 0 : ((two >> b) & 1u) ? 1 : ((three >> b) & 1u) ? 2 : 3);
        }
    }
}

// The tree as tracs_nj_edges gives it, nothing else: 2n - 3 edges in creation order, (n + t, a_t), (n + t, b_t) with a_t < b_t per
// join, then the top node with x < y < z; every node hangs under exactly one later node.
int fitch_tree_check(const char *who, size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges)
{
    const auto bad = [&](const char *what) { set_error(std::string(who) + ": " + what); return TRACS_E_ARG; };
    if (n < 1 || n > FITCH_MAX_N) return bad("the tree has between 1 and 2^21 leaves");
    const size_t want = n >= 3 ? 2 * n - 3 : n - 1;
    if (n_edges != want) return bad("a tree over n leaves has 2n - 3 edges");
    if (n_edges && (!parent || !child)) return bad("NULL argument");
    if (n == 1) return TRACS_OK;
    if (n == 2) return (parent[0] == 0 && child[0] == 1) ? TRACS_OK : bad("the tree of two leaves is the edge (0, 1)");
    const size_t J = n - 3, top = 2 * n - 3;
    std::vector<uint8_t> hung(top, 0);
    const auto hang = [&](size_t p, uint32_t c) {
        if (c >= p || hung[c]) return false;                               // (a child is older than its parent and hangs once)
        hung[c] = 1;
        return true;
    };
    for (size_t t = 0; t < J; t++) {
        if (parent[2 * t] != n + t || parent[2 * t + 1] != n + t || child[2 * t] >= child[2 * t + 1] || !hang(n + t, child[2 * t]) ||
            !hang(n + t, child[2 * t + 1]))
            return bad("the edges are not a tree in creation order");
    }
    for (size_t q = 0; q < 3; q++)
        if (parent[2 * J + q] != top || (q && child[2 * J + q - 1] >= child[2 * J + q]) || !hang(top, child[2 * J + q]))
            return bad("the edges are not a tree in creation order");
    return TRACS_OK;                                                       // (2n - 3 distinct children below 2n - 3: every node hangs)
}

int fitch_check(const tracs_alignment *a, const char *who)
{
    if (!a || !a->planes) { set_error(std::string(who) + ": NULL alignment"); return TRACS_E_ARG; }
    if (a->L >= (1ull << 31)) { set_error(std::string(who) + ": alignment longer than 2^31 sites"); return TRACS_E_ARG; }
    return TRACS_OK;
}

// The slabs of the groups [g_begin, g_end): the slab's length (at most max_slab groups when that is not 0), the node buffer and the
// child column on the device.  The tree was checked.
struct FitchSlabs {
    size_t slab = 0, stride = 0, W = 0, nodes = 0;
    uint4 *buf = nullptr;
    unsigned *d_child = nullptr;
};
int fitch_slabs(const tracs_alignment *a, const uint32_t *child, size_t n_edges, size_t g_begin, size_t g_end, size_t max_slab, FitchSlabs &S,
                hipStream_t stream)
{
    const size_t n = a->n, nodes = n >= 3 ? 2 * n - 2 : n;
    size_t slab = std::max<size_t>(1, FITCH_SLAB_BYTES / (nodes * 64));
    if (slab >= 16) slab &= ~(size_t)15;                                   // (whole waves of words)
    slab = std::max<size_t>(1, (size_t)sw::size(sw::TRACS_FITCH_SLAB_GROUPS, slab));
    slab = std::min(slab, g_end - g_begin);
    if (max_slab) slab = std::min(slab, max_slab);
    int rc;
    uint4 *buf = nullptr;
    while (!workspace_try(WS_FITCH_NODES, nodes * slab * 4, &buf)) {      // (no room for the budget: shorter slabs)
        if (slab == 1) return workspace_get(WS_FITCH_NODES, nodes * slab * 4, &buf);
        slab = std::max<size_t>(1, slab / 2);
    }
    unsigned *d_child = nullptr;
    if ((rc = workspace_get(WS_FITCH_TREE, std::max<size_t>(n_edges, 1), &d_child))) return rc;
    if (n_edges) {
        TRACS_HIP_CHECK(hipMemcpyAsync(d_child, child, n_edges * 4, hipMemcpyHostToDevice, stream));
        TRACS_HIP_CHECK(hipStreamSynchronize(stream));                     // (the edges are the caller's memory)
    }
    S.slab = slab; S.stride = slab * 4; S.W = (a->L + 31) / 32; S.nodes = nodes; S.buf = buf; S.d_child = d_child;
    return TRACS_OK;
}

// one slab from group g0: the leaves, then the walk; -> the waves (chunks) of the walk
template <int MODE>
size_t fitch_slab_launch(const tracs_alignment *a, const FitchSlabs &S, size_t g0, size_t g_end, size_t site_begin, size_t site_end,
                         unsigned *edge_changes, unsigned *site_changes, uint8_t *site_minimum, const long long *off, long long base, size_t room,
                         unsigned *site, unsigned *edge, unsigned *info, hipStream_t stream)
{
    const size_t n = a->n;
    const size_t sg = std::min(S.slab, g_end - g0);
    const size_t words = std::min(sg * 4, S.W - g0 * 4);
    const size_t waves = (words + 63) / 64;
    hipLaunchKernelGGL(fitch_leaves_kernel, dim3((unsigned)((sg + 3) / 4), (unsigned)((n + 63) / 64)), dim3(256), 0, stream, a->planes,
                       (unsigned)n, a->n_pad, g0, (unsigned)sg, S.buf, S.stride);
    hipLaunchKernelGGL(fitch_walk_kernel<MODE>, dim3((unsigned)waves), dim3(64), 0, stream, S.buf, S.stride, (unsigned)n, S.d_child,
                       (unsigned)(g0 * 4), (unsigned)words, (unsigned)site_begin, (unsigned)site_end, edge_changes, site_changes, site_minimum,
                       off, base, (long long)room, site, edge, info);
    return waves;
}

// Sites [site_begin, site_end) slab by slab: the leaves, then the walk.  The tree was checked.
template <int MODE>
int fitch_run(const tracs_alignment *a, const uint32_t *child, size_t n_edges, size_t site_begin, size_t site_end, unsigned *edge_changes,
              unsigned *site_changes, uint8_t *site_minimum, const long long *off, long long base, size_t room, unsigned *site, unsigned *edge,
              unsigned *info, hipStream_t stream)
{
    if (site_begin >= site_end) return TRACS_OK;
    const size_t g_begin = site_begin / SITES_PER_GROUP, g_end = groups_for(site_end);
    FitchSlabs S;
    int rc;
    if ((rc = fitch_slabs(a, child, n_edges, g_begin, g_end, 0, S, stream))) return rc;
    for (size_t g0 = g_begin; g0 < g_end; g0 += S.slab)
        fitch_slab_launch<MODE>(a, S, g0, g_end, site_begin, site_end, edge_changes, site_changes, site_minimum, off, base, room, site, edge, info,
                                stream);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

// Every column of a range's [chunks][n_edges] matrix from counts to bases: base[c][e] = cursor[e] + (the counts of the chunks before c);
// cursor[e] moves on by the range's sum.  One thread per edge: the loads of a step are coalesced across edges.
__global__ __launch_bounds__(256) void fitch_edge_scan_kernel(unsigned *__restrict__ matrix, size_t chunks, size_t n_edges,
                                                              unsigned *__restrict__ cursor)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    unsigned run = cursor[e];
    for (size_t c = 0; c < chunks; c++) {
        const unsigned v = matrix[c * n_edges + e];
        matrix[c * n_edges + e] = run;
        run += v;
    }
    cursor[e] = run;
}

// info |= 256 on the entries (site, edge) of a filled batch that `dropped` marks: the entry is looked up in its edge's ascending
// segment of edge_site.  An entry whose edge or site is not there is left alone.
__global__ __launch_bounds__(256) void fitch_mark_kernel(const unsigned *__restrict__ site, const unsigned *__restrict__ edge,
                                                         unsigned *__restrict__ info, size_t n_entries, size_t n_edges,
                                                         const long long *__restrict__ edge_off, const unsigned *__restrict__ edge_site,
                                                         const uint8_t *__restrict__ dropped)
{
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n_entries; k += (size_t)gridDim.x * 256) {
        const unsigned e = edge[k], s = site[k];
        if (e >= n_edges) continue;
        long long lo = edge_off[e];
        const long long end = edge_off[e + 1];
        long long hi = end;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (edge_site[mid] < s) lo = mid + 1; else hi = mid;
        }
        if (lo < end && edge_site[lo] == s && dropped[lo]) info[k] |= 256u;
    }
}

}  // namespace

// fitch_tree_check for the other files that take the tree of tracs_nj_edges (tree_mask.hip)
int nj_tree_check(const char *who, size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges)
{
    return fitch_tree_check(who, n, parent, child, n_edges);
}

// edge_changes[0 .. n_edges), site_changes[0 .. L), site_minimum[0 .. L), off[0 .. L] (device); *total (host) = off[L].  Synchronises.
int fitch_count(const tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, unsigned *edge_changes,
                unsigned *site_changes, uint8_t *site_minimum, long long *off, uint64_t *total, hipStream_t stream)
{
    if (total) *total = 0;
    int rc = fitch_check(a, "tracs_fitch_count");
    if (rc || (rc = fitch_tree_check("tracs_fitch_count", a->n, parent, child, n_edges))) return rc;
    if (!off || (n_edges && !edge_changes) || (a->L && (!site_changes || !site_minimum))) { set_error("tracs_fitch_count: NULL argument"); return TRACS_E_ARG; }
    DeviceCall guard(stream);
    unsigned long long *sums;
    if ((rc = workspace_get(WS_FITCH_SUMS, offsets_scan_sums(a->L), &sums))) return rc;
    if (n_edges) TRACS_HIP_CHECK(hipMemsetAsync(edge_changes, 0, n_edges * 4, stream));
    if ((rc = fitch_run<FITCH_COUNT>(a, child, n_edges, 0, a->L, edge_changes, site_changes, site_minimum, nullptr, 0, 0, nullptr, nullptr, nullptr, stream)) ||
        (rc = offsets_scan_launch(site_changes, a->L, sums, off, stream))) return rc;
    long long tot = 0;
    TRACS_HIP_CHECK(hipMemcpyAsync(&tot, off + a->L, 8, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    if (total) *total = (uint64_t)tot;
    return TRACS_OK;
}

// The entries of sites [site_begin, site_end) at site / edge / info [off[s] - base, off[s + 1] - base) (room: entries the buffers hold)
int fitch_fill(const tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, size_t site_begin, size_t site_end,
               const long long *off, long long base, unsigned *site, unsigned *edge, unsigned *info, size_t room, hipStream_t stream)
{
    int rc = fitch_check(a, "tracs_fitch_fill");
    if (rc || (rc = fitch_tree_check("tracs_fitch_fill", a->n, parent, child, n_edges))) return rc;
    if (site_begin > site_end || site_end > a->L) { set_error("tracs_fitch_fill: site range outside the alignment"); return TRACS_E_ARG; }
    if (site_begin == site_end || !room || !n_edges) return TRACS_OK;
    if (!off || !site || !edge || !info) { set_error("tracs_fitch_fill: NULL argument"); return TRACS_E_ARG; }
    DeviceCall guard(stream);
    return fitch_run<FITCH_FILL>(a, child, n_edges, site_begin, site_end, nullptr, nullptr, nullptr, off, base, room, site, edge, info, stream);
}

// The changes regrouped by edge.  edge_changes: fitch_count's (device); edge_off[0 .. n_edges] <- its exclusive scan;
// edge_site[edge_off[e] .. edge_off[e + 1]) <- the sites with a change on e, ascending; nothing is stored outside [0, room).
// The [chunk][edge] matrix holds a range of whole slabs at a time (FITCH_MATRIX_BYTES; TRACS_FITCH_MATRIX_CHUNKS: chunks per range,
// diagnostic -- it also shortens the slab to that many chunks).
int fitch_edge_sites(const tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, const unsigned *edge_changes,
                     long long *edge_off, unsigned *edge_site, size_t room, hipStream_t stream)
{
    int rc = fitch_check(a, "tracs_fitch_edge_sites");
    if (rc || (rc = fitch_tree_check("tracs_fitch_edge_sites", a->n, parent, child, n_edges))) return rc;
    if (!edge_off || (n_edges && !edge_changes) || (room && !edge_site)) { set_error("tracs_fitch_edge_sites: NULL argument"); return TRACS_E_ARG; }
    DeviceCall guard(stream);
    if (!n_edges) {
        TRACS_HIP_CHECK(hipMemsetAsync(edge_off, 0, 8, stream));
        return TRACS_OK;
    }
    unsigned long long *sums;
    if ((rc = workspace_get(WS_FITCH_SUMS, offsets_scan_sums(std::max<size_t>(n_edges, a->L)), &sums)) ||
        (rc = offsets_scan_launch(edge_changes, n_edges, sums, edge_off, stream))) return rc;
    if (!room || !a->L) return TRACS_OK;
    const size_t g_end = groups_for(a->L);
    const size_t range_chunks = std::max<size_t>(1, (size_t)sw::size(sw::TRACS_FITCH_MATRIX_CHUNKS, FITCH_MATRIX_BYTES / (n_edges * 4)));
    FitchSlabs S;
    // (a slab of g groups walks ceil(g / 16) chunks: one that outgrows the range is cut to whole chunks)
    if ((rc = fitch_slabs(a, child, n_edges, 0, g_end, range_chunks * FITCH_CHUNK_GROUPS, S, stream))) return rc;
    const size_t slab_chunks = (S.slab * 4 + 63) / 64;
    const size_t range_slabs = std::max<size_t>(1, range_chunks / slab_chunks);
    const size_t total_slabs = (g_end + S.slab - 1) / S.slab;
    unsigned *matrix, *cursor;
    if ((rc = workspace_get(WS_FITCH_MATRIX, std::min(range_slabs, total_slabs) * slab_chunks * n_edges, &matrix)) ||
        (rc = workspace_get(WS_FITCH_CURSOR, n_edges, &cursor))) return rc;
    TRACS_HIP_CHECK(hipMemsetAsync(cursor, 0, n_edges * 4, stream));
    for (size_t r0 = 0; r0 < g_end; r0 += range_slabs * S.slab) {
        const size_t r1 = std::min(g_end, r0 + range_slabs * S.slab);
        size_t chunks = 0;
        for (size_t g0 = r0; g0 < r1; g0 += S.slab)
            chunks += fitch_slab_launch<FITCH_ECOUNT>(a, S, g0, g_end, 0, a->L, matrix + chunks * n_edges, nullptr, nullptr, nullptr, 0, 0, nullptr,
                                                      nullptr, nullptr, stream);
        hipLaunchKernelGGL(fitch_edge_scan_kernel, dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, stream, matrix, chunks, n_edges, cursor);
        chunks = 0;
        for (size_t g0 = r0; g0 < r1; g0 += S.slab)
            chunks += fitch_slab_launch<FITCH_EFILL>(a, S, g0, g_end, 0, a->L, matrix + chunks * n_edges, nullptr, nullptr, edge_off, 0, room, edge_site,
                                                     nullptr, nullptr, stream);
    }
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

// Bit 8 of info on the entries of a filled batch that the branch filter drops (tracs_fitch_mark_dropped)
int fitch_mark_dropped(const unsigned *site, const unsigned *edge, unsigned *info, size_t n_entries, size_t n_edges, const long long *edge_off,
                       const unsigned *edge_site, const uint8_t *dropped, hipStream_t stream)
{
    if (!n_entries) return TRACS_OK;
    if (!site || !edge || !info || !edge_off || !edge_site || !dropped) { set_error("tracs_fitch_mark_dropped: NULL argument"); return TRACS_E_ARG; }
    const unsigned blocks = (unsigned)std::min<size_t>((n_entries + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(fitch_mark_kernel, dim3(blocks), dim3(256), 0, stream, site, edge, info, n_entries, n_edges, edge_off, edge_site, dropped);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

// ---- the rows of --tree-changes and --tree-sites ---------------------------------------------------------------------------------------
static inline void fitch_append_u64(std::string &s, uint64_t v)
{
    char buf[24];
    int k = 24;
    do { buf[--k] = (char)('0' + v % 10); v /= 10; } while (v);
    s.append(buf + k, 24 - k);
}

// The count pass for the handle's tree; what the writer needs stays in `t` (the device arrays; on the host the edges' counts, the
// offsets and the minimum).  sum_minimum: over the sites with a change.
int fitch_tables(const tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, FitchTables &t)
{
    int rc = fitch_check(a, "tracs_distance_tree_changes");
    if (rc) return rc;
    const size_t L = a->L;
    if ((rc = t.d_edge.alloc(std::max<size_t>(n_edges, 1), "changes by edge")) || (rc = t.d_site.alloc(std::max<size_t>(L, 1), "changes by site")) ||
        (rc = t.d_min.alloc(std::max<size_t>(L, 1), "site minimum")) || (rc = t.d_off.alloc(L + 1, "site offsets"))) return rc;
    if ((rc = fitch_count(a, parent, child, n_edges, t.d_edge.get(), t.d_site.get(), t.d_min.get(), t.d_off.get(), &t.total, nullptr))) return rc;
    t.edge_changes.assign(n_edges, 0);
    t.off.assign(L + 1, 0);
    t.minimum.assign(L, 0);
    if (n_edges) TRACS_HIP_CHECK(hipMemcpy(t.edge_changes.data(), t.d_edge.get(), n_edges * 4, hipMemcpyDeviceToHost));
    TRACS_HIP_CHECK(hipMemcpy(t.off.data(), t.d_off.get(), (L + 1) * 8, hipMemcpyDeviceToHost));
    if (L) TRACS_HIP_CHECK(hipMemcpy(t.minimum.data(), t.d_min.get(), L, hipMemcpyDeviceToHost));
    t.sum_minimum = 0;
    for (size_t s = 0; s < L; s++) if (t.off[s + 1] > t.off[s]) t.sum_minimum += t.minimum[s];
    return TRACS_OK;
}

// After fitch_tables: the change rows appended to changes_path (may be NULL) and the site rows to sites_path (may be NULL).  The
// entries come in batches of sites: device entry buffer -> pinned host buffer -> rows formatted on host threads and appended in order.
// The two buffers hold at most 256 MiB each (TRACS_FITCH_BATCH: entries per batch instead, for tests), or one site's entries when a
// site has more.  kept / source_len / contigs: as pair_sites_write.  flt != NULL (--tree-filter): every batch is marked
// with the branch filter's verdicts and the change rows carry a dropped field (0 / 1) before ref.
int fitch_write(const tracs_alignment *a, const char *const *names, const uint64_t *kept, size_t source_len, const uint32_t *parent,
                const uint32_t *child, size_t n_edges, const FitchTables &t, const char *changes_path, const char *sites_path, const char *ref,
                const char *const *contig_names, const uint64_t *contig_lengths, size_t n_contigs, int n_threads, const FitchFilter *flt)
{
    const size_t n = a->n, L = a->L;
    if (!names || !ref || (n_contigs && (!contig_names || !contig_lengths))) { set_error("tracs_distance_tree_changes: NULL argument"); return TRACS_E_ARG; }
    std::vector<uint64_t> src_col;                                         // kept column -> column of the files read
    if (kept) {
        src_col.reserve(L);
        for (size_t s = 0; s < source_len; s++)
            if ((kept[s >> 6] >> (s & 63)) & 1ull) src_col.push_back(s);
        if (src_col.size() != L) { set_error("tracs_distance_tree_changes: the kept-columns bitmap does not match the alignment"); return TRACS_E_ARG; }
    }
    std::vector<uint64_t> contig_end(n_contigs);
    { uint64_t o = 0; for (size_t c = 0; c < n_contigs; c++) { o += contig_lengths[c]; contig_end[c] = o; } }
    if (n_contigs && L) {
        const uint64_t last = kept ? src_col.back() : L - 1;
        if (last >= contig_end.back()) {
            set_error("the alignment reaches column " + std::to_string(last) + ", past the reference's contigs (" + std::to_string(contig_end.back()) + ")");
            return TRACS_E_ARG;
        }
    }
    // "contig,position" of a packed site
    const auto append_place = [&](std::string &s, size_t packed) {
        const uint64_t col = kept ? src_col[packed] : packed;
        if (n_contigs) {
            const size_t c = (size_t)(std::upper_bound(contig_end.begin(), contig_end.end(), col) - contig_end.begin());
            s += contig_names[c];
            s += ',';
            fitch_append_u64(s, col - (c ? contig_end[c - 1] : 0));
        } else {
            s += "alignment,";
            fitch_append_u64(s, col);
        }
    };
    const auto append_file = [&](const char *path, const std::string &text, FILE *&fp) {
        if (!text.empty() && std::fwrite(text.data(), 1, text.size(), fp) != text.size()) { set_error(std::string("write error on ") + path); return TRACS_E_OPEN; }
        return TRACS_OK;
    };
    int rc = TRACS_OK;
    if (sites_path) {
        FILE *fp = std::fopen(sites_path, "ab");
        if (!fp) { set_error(std::string("cannot open ") + sites_path + " for appending"); return TRACS_E_OPEN; }
        std::string text;
        for (size_t s = 0; s < L && !rc; s++) {
            const long long c = t.off[s + 1] - t.off[s];
            if (c <= 0) continue;
            append_place(text, s);
            text += ',';
            fitch_append_u64(text, (uint64_t)c);
            text += ',';
            fitch_append_u64(text, t.minimum[s]);
            text += ',';
            text += ref;
            text += '\n';
            if (text.size() >= (1u << 20)) { rc = append_file(sites_path, text, fp); text.clear(); }
        }
        if (!rc) rc = append_file(sites_path, text, fp);
        if (std::fclose(fp) != 0 && !rc) { set_error(std::string("write error on ") + sites_path); rc = TRACS_E_OPEN; }
        if (rc) return rc;
    }
    if (!changes_path) return TRACS_OK;
    DeviceCall guard(nullptr);
    DeviceArray<unsigned> ent_buf;
    PinnedArray<unsigned> host_buf;
    const std::vector<long long> &off = t.off;
    const uint64_t total = t.total;
    const size_t cap = std::max<size_t>(1, (size_t)sw::size(sw::TRACS_FITCH_BATCH, (256ull << 20) / 12));         // entries per batch: 12 bytes each
    long long max_c = 0;
    for (size_t s = 0; s < L; s++) max_c = std::max(max_c, off[s + 1] - off[s]);
    const size_t room = std::max<size_t>(std::max<size_t>(std::min<size_t>(cap, total), (size_t)max_c), 1);
    if (total && ((rc = ent_buf.alloc(room * 3, "tree-change entries")) || (rc = host_buf.alloc(room * 3, "tree-change entries")))) return rc;
    unsigned *const d_ent = ent_buf.get(), *const h_ent = host_buf.get();
    std::unique_ptr<FILE, int (*)(FILE *)> file(std::fopen(changes_path, "ab"), std::fclose);
    FILE *fp = file.get();
    if (!fp) { set_error(std::string("cannot open ") + changes_path + " for appending"); return TRACS_E_OPEN; }
    // "parent,child," of every edge (internal node n + t is "#t+1", as in the edge rows)
    std::vector<std::string> head(n_edges);
    for (size_t e = 0; e < n_edges; e++) {
        for (const uint32_t v : {parent[e], child[e]}) {
            if (v < n) head[e] += names[v];
            else { head[e] += '#'; head[e] += std::to_string((size_t)v - n + 1); }
            head[e] += ',';
        }
    }
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const size_t n_thr = n_threads > 0 ? std::min<size_t>((size_t)n_threads, 64) : hw;
    const size_t slice = 1u << 18;                                         // entries one thread formats at a time
    static const char letters[] = "XACXGXXXTXXXXXXX";                      // (the states are one-hot)
    std::vector<std::string> text(n_thr);
    for (size_t s0 = 0; s0 < L && total;) {
        size_t s1 = s0 + 1;                                                // (a batch is never less than one site)
        while (s1 < L && (size_t)(off[s1 + 1] - off[s0]) <= cap) s1++;
        const long long base = off[s0];
        const size_t entries = (size_t)(off[s1] - base);
        if (entries) {
            if ((rc = fitch_fill(a, parent, child, n_edges, s0, s1, t.d_off.get(), base, d_ent, d_ent + room, d_ent + 2 * room, room, nullptr))) return rc;
            if (flt && (rc = fitch_mark_dropped(d_ent, d_ent + room, d_ent + 2 * room, entries, n_edges, flt->d_edge_off, flt->d_edge_site,
                                                flt->d_dropped, nullptr))) return rc;
            for (int q = 0; q < 3; q++) TRACS_HIP_CHECK(hipMemcpy(h_ent + q * room, d_ent + q * room, entries * 4, hipMemcpyDeviceToHost));
            const unsigned *h_site = h_ent, *h_edge = h_ent + room, *h_info = h_ent + 2 * room;
            auto format = [&](size_t k, size_t e0, size_t e1) {
                std::string &s = text[k];
                s.clear();
                for (size_t e = e0; e < e1; e++) {
                    const unsigned v = h_info[e];
                    if (h_edge[e] >= n_edges || h_site[e] >= L) continue;  // (never: the fill writes every entry of the batch)
                    s += head[h_edge[e]];
                    append_place(s, h_site[e]);
                    s += ',';
                    s += letters[v & 15u];
                    s += ',';
                    s += letters[(v >> 4) & 15u];
                    s += ',';
                    if (flt) { s += (v & 256u) ? '1' : '0'; s += ','; }
                    s += ref;
                    s += '\n';
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
                    if ((rc = append_file(changes_path, text[k], fp))) return rc;
            }
        }
        s0 = s1;
    }
    if (std::fclose(file.release()) != 0) { set_error(std::string("write error on ") + changes_path); return TRACS_E_OPEN; }
    return TRACS_OK;
}

}  // namespace tracs

using namespace tracs;

extern "C" {

int tracs_fitch_count(const tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, uint32_t *edge_changes,
                      uint32_t *site_changes, uint8_t *site_minimum, int64_t *off, uint64_t *total, void *stream)
{
    return fitch_count(a, parent, child, n_edges, edge_changes, site_changes, site_minimum, reinterpret_cast<long long *>(off), total,
                       static_cast<hipStream_t>(stream));
}

int tracs_fitch_fill(const tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, size_t site_begin, size_t site_end,
                     const int64_t *off, int64_t entry_base, uint32_t *site, uint32_t *edge, uint32_t *info, size_t room, void *stream)
{
    return fitch_fill(a, parent, child, n_edges, site_begin, site_end, reinterpret_cast<const long long *>(off), (long long)entry_base, site, edge,
                      info, room, static_cast<hipStream_t>(stream));
}

int tracs_fitch_edge_sites(const tracs_alignment *a, const uint32_t *parent, const uint32_t *child, size_t n_edges, const uint32_t *edge_changes,
                           int64_t *edge_off, uint32_t *edge_site, size_t room, void *stream)
{
    return fitch_edge_sites(a, parent, child, n_edges, edge_changes, reinterpret_cast<long long *>(edge_off), edge_site, room,
                            static_cast<hipStream_t>(stream));
}

int tracs_fitch_mark_dropped(const uint32_t *site, const uint32_t *edge, uint32_t *info, size_t n_entries, size_t n_edges, const int64_t *edge_off,
                             const uint32_t *edge_site, const uint8_t *dropped, void *stream)
{
    DeviceCall guard(static_cast<hipStream_t>(stream));
    return fitch_mark_dropped(site, edge, info, n_entries, n_edges, reinterpret_cast<const long long *>(edge_off), edge_site, dropped,
                              static_cast<hipStream_t>(stream));
}

}  // extern "C"
