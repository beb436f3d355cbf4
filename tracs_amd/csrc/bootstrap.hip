// bootstrap.hip -- bootstrap replicates of an alignment: which columns a replicate draws, and the replicate's packed planes.
//
// One replicate is, by definition, the run on an alignment whose columns were drawn with replacement: column c of the source repeated
// w(c) times, columns in ascending c.  The replicate is packed into a NEW handle that is byte for byte what packing that text gives, so
// everything downstream (pair kernels, site classes, neighbour joining) runs on it unchanged.
//
//     bootstrap_weights_kernel   one thread per draw t: c(b, t) from the counter-based generator, an integer atomic on w(c)
//     widen_weights_kernel       uint32 weights -> int64 counts for scan_i64_inplace_kernel (scan_kernels.h): off[c] = the first output
//                                column of source column c, off[L] = the replicate's length
//     gather_starts_kernel       per output group of 128 columns, the source column of its first column (a search in the offsets)
//     gather_sites_kernel        the five planes of the replicate
//
// and, on the host, the comparison of two trees' splits (tracs_tree_support).
#include "common.h"
#include "scan_kernels.h"
#include "debug_api.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>

namespace tracs {

// ---------------------------------------------------------------------------------------------------------------------------------
// The draws.  mix = the splitmix64 finaliser; key_b = mix(S + G (b + 1)); u(b, t) = mix(key_b + G (t + 1)); c = (u L) >> 64.
constexpr unsigned long long BS_GOLDEN = 0x9E3779B97F4A7C15ull;
__host__ __device__ __forceinline__ unsigned long long bs_mix(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// One thread per draw.  bits == NULL: weights is L long and takes every draw (the definition's form).  Else bits / woff are the
// differing-columns bitmap in 32-column words and the rank of each word's first differing column: weights is V long, indexed by the
// rank among the differing columns, and a draw of any other column is dropped (it adds nothing to any distance).  The counts are integer
// sums: the order of the atomics cannot show.
__global__ __launch_bounds__(256) void bootstrap_weights_kernel(unsigned long long L, unsigned long long key, const unsigned *__restrict__ bits,
                                                                const unsigned *__restrict__ woff, unsigned *__restrict__ weights)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= L) return;
    const unsigned long long u = bs_mix(key + BS_GOLDEN * (t + 1));
    const unsigned long long c = __umul64hi(u, L);                      // < L
    if (bits == nullptr) { atomicAdd(&weights[c], 1u); return; }
    const unsigned word = bits[c >> 5], bit = (unsigned)c & 31u;
    if ((word >> bit) & 1u) atomicAdd(&weights[woff[c >> 5] + __popc(word & ((1u << bit) - 1u))], 1u);
}

int bootstrap_weights_launch(size_t L, uint64_t seed, uint64_t replicate, const unsigned *bits, const unsigned *woff, uint32_t *weights,
                             size_t weights_len, hipStream_t stream)
{
    if (!L || !weights_len) return TRACS_OK;
    if ((L + 255) / 256 > 0x7FFFFFFFull) { set_error("tracs_bootstrap_weights: too many columns"); return TRACS_E_ARG; }
    const unsigned long long key = bs_mix(seed + BS_GOLDEN * (replicate + 1));
    TRACS_HIP_CHECK(hipMemsetAsync(weights, 0, weights_len * 4, stream));
    hipLaunchKernelGGL(bootstrap_weights_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, stream, (unsigned long long)L, key, bits, woff, weights);
    TRACS_HIP_CHECK(hipGetLastError());
    return TRACS_OK;
}

__global__ __launch_bounds__(256) void widen_weights_kernel(const unsigned *__restrict__ w, size_t L, long long *__restrict__ off)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c < L) off[c] = (long long)w[c];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The source column of every output group's first column: the last c with off[c] <= 128 G (off[0] = 0 <= 128 G < total = off[L_src], so
// c stays in [0, L_src) and w(c) > 0).  One thread per output group: the ~log2 L dependent loads of the search are paid once per
// group here, not once per (group, 64 samples) in the gather.
__global__ __launch_bounds__(256) void gather_starts_kernel(const long long *__restrict__ off, unsigned L_src, unsigned groups_dst,
                                                            unsigned *__restrict__ first)
{
    const unsigned G = blockIdx.x * 256 + threadIdx.x;
    if (G >= groups_dst) return;
    const unsigned long long pos0 = (unsigned long long)G * SITES_PER_GROUP;
    unsigned lo = 0, hi = L_src;
    while (hi - lo > 1) {
        const unsigned mid = lo + (hi - lo) / 2;
        if ((unsigned long long)off[mid] <= pos0) lo = mid; else hi = mid;
    }
    first[G] = lo;
}

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, unsigned k)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, (int)k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), (int)k);
    return ((unsigned long long)hi << 32) | lo;
}

// Gather: one thread = one (sample, OUTPUT group of 128 replicate columns), lanes over samples like select_sites_kernel, so the source
// column, its word, its shift and every output mask are wave-uniform and live on the scalar unit.  The walk starts at first[G] and
// goes up the source columns through the scanned counts (source column c fills the output columns [off[c], off[c + 1])): a search in
// the offsets, not an expanded index list -- the list would cost 4 bytes per output column to write and to read back, the offsets
// are 8 bytes per SOURCE column and there already.  The offsets come in windows of 64, one per lane in a single coalesced load, and
// the walk takes them out with v_readlane: one memory latency per 64 source columns.  A column with w = 0 costs one compare.  A column
// with w > 0 fills the output bits [pos, pos + w): the lane's bit of that column is widened to a full word per plane once, and the run
// is cut at the output words' boundaries -- per (run, output word) one mask on the scalar unit and an AND and an OR per plane into the
// word being collected (cur[]), which goes into out[][] when the walk leaves it.  So w = 300 is ten words, each as cheap as a run of
// one bit, and the usual run (w = 1 .. 3, inside one word) costs ~4 vector operations per plane.  (The first form ORed every run
// into all four output words of every plane under four masks, ~14 operations per plane and run: 42 ms for 10 000 samples x 3.1 M
// columns where this one takes 23, DESIGN.md 3.18 -- the kernel is bound by its instruction stream, not by the offsets' latency:
// scalar loads of the offsets, one per column, in place of the windows made no difference to the first form.)  A source group is
// loaded once per thread while the walk stays inside it (five 16-byte loads per lane, 1 KiB per wave and plane, coalesced) and a
// source word is picked out of it once per 32 source columns, whatever the weights: never per output bit.  Reads 5 x 16 bytes per
// sample and source group with a drawn column, writes 5 x 16 bytes per sample and output group; tail bits of the last group stay
// zero, pad samples are not written (the handle was cleared when it was created); N = A & C & G & T holds per column, so it holds
// for the copies.
// (Every lane of a wave is active throughout: n_pad is a multiple of 64 and the grid covers it exactly, so readlane never reads an
// inactive lane.)
__global__ __launch_bounds__(256) void gather_sites_kernel(const uint4 *__restrict__ src, const long long *__restrict__ off,
                                                           const unsigned *__restrict__ first, unsigned L_src, unsigned long long total,
                                                           uint4 *__restrict__ dst, size_t n_pad, unsigned s_first, unsigned n, unsigned groups_dst)
{
    const unsigned lane = threadIdx.x & 63;
    const unsigned s = s_first + blockIdx.y * 64 + lane;
    const unsigned G = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (G >= groups_dst) return;                                          // (wave-uniform; s < n_pad by the grid)
    const unsigned long long pos0 = (unsigned long long)G * SITES_PER_GROUP;
    const unsigned long long end = min(pos0 + SITES_PER_GROUP, total);
    unsigned c = __builtin_amdgcn_readfirstlane(first[G]), held = 0xFFFFFFFFu, heldw = 0xFFFFFFFFu;
    unsigned c0 = c;                                                      // the window: lane l holds off[c0 + 1 + l] (clamped to off[L_src])
    unsigned long long win = (unsigned long long)off[min(c0 + 1u + lane, L_src)];
    unsigned long long pos = pos0;
    uint4 v[NPLANES];
    unsigned xw[NPLANES], cur[NPLANES], out[NPLANES][4];
#pragma unroll
    for (int p = 0; p < NPLANES; p++) {
        v[p] = make_uint4(0, 0, 0, 0);
        xw[p] = cur[p] = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) out[p][q] = 0;
    }
    unsigned ow = 0;                                                      // the output word cur[] collects (wave-uniform)
    auto flush = [&]() {
#pragma unroll
        for (int p = 0; p < NPLANES; p++)
#pragma unroll
            for (int q = 0; q < 4; q++) out[p][q] = ow == (unsigned)q ? cur[p] : out[p][q];      // (selects: out[][] is only ever indexed by constants)
    };
    while (pos < end) {                                                   // (c + 1 <= L_src while pos < total)
        if (c - c0 >= 64u) {
            c0 = c;
            win = (unsigned long long)off[min(c0 + 1u + lane, L_src)];
        }
        const unsigned long long nxt = readlane64(win, __builtin_amdgcn_readfirstlane(c - c0));      // off[c + 1]
        if (nxt <= pos) { c++; continue; }                                // w(c) = 0
        const unsigned long long run_end = min(nxt, end);
        const unsigned sw = c >> 5;
        if (sw != heldw) {                                                // a new source word: at most once per 32 source columns
            const unsigned g = c >> 7, wq = sw & 3u;
            if (g != held) {
#pragma unroll
                for (int p = 0; p < NPLANES; p++) v[p] = src[((size_t)g * NPLANES + p) * n_pad + s];
                held = g;
            }
#pragma unroll
            for (int p = 0; p < NPLANES; p++) xw[p] = wq == 0 ? v[p].x : wq == 1 ? v[p].y : wq == 2 ? v[p].z : v[p].w;
            heldw = sw;
        }
        const unsigned up = 31u - (c & 31u);
        unsigned full[NPLANES];                                           // the lane's bit of column c in every bit of a word
#pragma unroll
        for (int p = 0; p < NPLANES; p++) full[p] = (unsigned)((int)(xw[p] << up) >> 31);
        // the run's output bits [b0, b1), one output word at a time (w = 300 is ten words, each as cheap as a run of one bit)
        unsigned b0 = (unsigned)(pos - pos0);
        const unsigned b1 = (unsigned)(run_end - pos0);
        while (b0 < b1) {
            const unsigned q = b0 >> 5;
            if (q != ow) {
                flush();
#pragma unroll
                for (int p = 0; p < NPLANES; p++) cur[p] = 0;
                ow = q;
            }
            const unsigned e = min(b1, (q + 1u) * 32u), len = e - b0;
            const unsigned m = (len == 32u ? 0xFFFFFFFFu : ((1u << len) - 1u)) << (b0 & 31u);
#pragma unroll
            for (int p = 0; p < NPLANES; p++) cur[p] |= full[p] & m;
            b0 = e;
        }
        pos = run_end;
        if (nxt == run_end) c++;
    }
    flush();
    if (s < n)
#pragma unroll
        for (int p = 0; p < NPLANES; p++)
            dst[((size_t)G * NPLANES + p) * n_pad + s] = make_uint4(out[p][0], out[p][1], out[p][2], out[p][3]);
}

// The replicate of `src` under `weights` (device uint32[src->L]) in a new handle (include/tracs_hip.h: tracs_alignment_gather_sites).
// empty_ok: a sum of 0 is not an error, *out stays NULL and *n_out 0 (tracs_distance_tree_bootstrap: the zero matrix).  stage_s
// (measurement, scripts/bench_bootstrap.py): the device is drained after each stage and its wall time goes to stage_s[0 .. 2] = the
// scan (with the groups' starts), the new handle, the gather kernel.
int gather_sites(const tracs_alignment *src, const uint32_t *weights, tracs_alignment **out, size_t *n_out, hipStream_t stream, bool empty_ok,
                 double *stage_s)
{
    auto t_last = std::chrono::steady_clock::now();
    auto stage = [&](int k) {
        if (!stage_s) return;
        (void)hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        stage_s[k] = std::chrono::duration<double>(now - t_last).count();
        t_last = now;
    };
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    if (!src || !out || (!weights && src->L)) { set_error("tracs_alignment_gather_sites: NULL argument"); return TRACS_E_ARG; }
    const size_t L = src->L;
    if (L >= 0xFFFFFFFFull) { set_error("tracs_alignment_gather_sites: too many columns"); return TRACS_E_ARG; }
    if (!L || !src->n) {
        if (empty_ok) return TRACS_OK;
        set_error("tracs_alignment_gather_sites: no column drawn");
        return TRACS_E_ARG;
    }
    DeviceCall guard(stream);
    long long *off = nullptr;
    unsigned *first = nullptr;
    int rc;
    if ((rc = workspace_get(WS_BS_OFFSETS, L + 1, &off))) return rc;
    hipLaunchKernelGGL(widen_weights_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, stream, weights, L, off);
    hipLaunchKernelGGL(scan_i64_inplace_kernel, dim3(1), dim3(1024), 0, stream, off, L);
    TRACS_HIP_CHECK(hipGetLastError());
    long long total = 0;
    TRACS_HIP_CHECK(hipMemcpyAsync(&total, off + L, 8, hipMemcpyDeviceToHost, stream));
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    if (total <= 0) {
        if (empty_ok) return TRACS_OK;
        set_error("tracs_alignment_gather_sites: no column drawn");
        return TRACS_E_ARG;
    }
    if ((unsigned long long)total >= (1ull << 32)) {
        set_error("tracs_alignment_gather_sites: the weights sum to " + std::to_string(total) + " columns, 2^32 or more");
        return TRACS_E_ARG;
    }
    const unsigned groups_dst = (unsigned)groups_for((size_t)total);
    if ((rc = workspace_get(WS_BS_STARTS, groups_dst, &first))) return rc;
    hipLaunchKernelGGL(gather_starts_kernel, dim3((groups_dst + 255) / 256), dim3(256), 0, stream, off, (unsigned)L, groups_dst, first);
    TRACS_HIP_CHECK(hipGetLastError());
    stage(0);
    tracs_alignment *made = nullptr;
    if ((rc = tracs_alignment_create(src->n, (size_t)total, &made))) return rc;
    AlignmentOwner dst(made);
    TRACS_HIP_CHECK(hipStreamSynchronize(nullptr));               // the new planes are cleared on the null stream
    stage(1);
    const size_t blocks_y = src->n_pad / 64, slice = 65535;
    for (size_t y0 = 0; y0 < blocks_y; y0 += slice) {
        const dim3 grid((groups_dst + 3) / 4, (unsigned)std::min(slice, blocks_y - y0));
        hipLaunchKernelGGL(gather_sites_kernel, grid, dim3(256), 0, stream, src->planes, off, first, (unsigned)L, (unsigned long long)total, dst->planes,
                           src->n_pad, (unsigned)(y0 * 64), (unsigned)src->n, groups_dst);
    }
    TRACS_HIP_CHECK(hipGetLastError());
    TRACS_HIP_CHECK(hipStreamSynchronize(stream));
    stage(2);
    if (n_out) *n_out = (size_t)total;
    *out = dst.release();
    return TRACS_OK;
}

// Host only.  below[v]: the leaves under internal node v as a bitset of ceil(n / 64) words, built bottom-up in the edges' creation order
// (a child's edges come before the edge that hangs it under its parent).  below == NULL: the edges are checked only; kids != NULL:
// <- the number of children of every node (transfer.hip, which wants two per joined node and three at the top).
int tree_bitsets(const char *who, size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges, std::vector<uint64_t> *below,
                 std::vector<uint32_t> *kids)
{
    const size_t W = (n + 63) / 64, n_nodes = 2 * n - 2;
    if (n_edges != 2 * n - 3) { set_error(std::string(who) + ": a tree over n leaves has 2n - 3 edges"); return TRACS_E_ARG; }
    if (below) below->assign((n_nodes - n) * W, 0);
    if (kids) kids->assign(n_nodes, 0);
    std::vector<uint8_t> open(n_nodes, 0), hung(n_nodes, 0);              // open: has children; hung: is somebody's child
    for (size_t e = 0; e < n_edges; e++) {
        const uint32_t p = parent[e], c = child[e];
        if (p < n || p >= n_nodes || c >= n_nodes || c == p || hung[c] || hung[p] || (c >= n && !open[c])) {
            set_error(std::string(who) + ": the edges are not a tree in creation order");
            return TRACS_E_ARG;
        }
        if (below) {
            uint64_t *bp = &(*below)[(p - n) * W];
            if (c < n) bp[c >> 6] |= 1ull << (c & 63);
            else { const uint64_t *bc = &(*below)[(c - n) * W]; for (size_t w = 0; w < W; w++) bp[w] |= bc[w]; }
        }
        if (kids) (*kids)[p]++;
        open[p] = 1;
        hung[c] = 1;
    }
    return TRACS_OK;
}

size_t bootstrap_column_words(const uint64_t *differs, size_t L, std::vector<unsigned> &bits, std::vector<unsigned> &woff)
{
    const size_t words = (L + 31) / 32;
    bits.resize(words); woff.resize(words);
    unsigned run = 0;
    for (size_t w = 0; w < words; w++) {
        bits[w] = (unsigned)(differs[w >> 1] >> (32 * (w & 1)));
        woff[w] = run;
        run += (unsigned)__builtin_popcount(bits[w]);
    }
    return run;
}

}  // namespace tracs

using namespace tracs;

extern "C" {

int tracs_bootstrap_weights(size_t L, uint64_t seed, uint64_t replicate, uint32_t *weights, void *stream_)
{
    if (!weights && L) { set_error("tracs_bootstrap_weights: NULL argument"); return TRACS_E_ARG; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DeviceCall guard(stream);
    return bootstrap_weights_launch(L, seed, replicate, nullptr, nullptr, weights, L, stream);
}

int tracs_alignment_gather_sites(const tracs_alignment *src, const uint32_t *weights, tracs_alignment **out, size_t *n_out, void *stream)
{
    return gather_sites(src, weights, out, n_out, static_cast<hipStream_t>(stream), false, nullptr);
}

// Measurement (scripts/bench_bootstrap.py): one replicate as tracs_distance_tree_bootstrap makes it, stage by stage with the device
// drained after each.  var: the differing columns of an alignment of L columns (tracs_alignment_select_sites under `differs`, the
// census bitmap, ceil(L / 64) host words).  seconds[4] <- the weights over the differing columns, the scan, the new handle, the gather
// kernel.  *out: the replicate (NULL when it drew no differing column), *n_out its length.
int tracs_debug_bootstrap_replicate(const tracs_alignment *var, size_t L, const uint64_t *differs, uint64_t seed, uint64_t replicate,
                                    double *seconds, tracs_alignment **out, size_t *n_out)
{
    if (out) *out = nullptr;
    if (!var || !differs || !seconds || !out || !L) { set_error("tracs_debug_bootstrap_replicate: bad argument"); return TRACS_E_ARG; }
    const size_t words = (L + 31) / 32, V = var->L;
    std::vector<unsigned> bits, woff;
    if (bootstrap_column_words(differs, L, bits, woff) != V) { set_error("tracs_debug_bootstrap_replicate: the bitmap does not have the handle's columns"); return TRACS_E_ARG; }
    DeviceArray<unsigned> buf;
    int rc = buf.alloc(2 * words + V, "replicate bitmap and weights");
    if (rc) return rc;
    unsigned *const d = buf.get();
    TRACS_HIP_CHECK(hipMemcpy(d, bits.data(), words * 4, hipMemcpyHostToDevice));
    TRACS_HIP_CHECK(hipMemcpy(d + words, woff.data(), words * 4, hipMemcpyHostToDevice));
    TRACS_HIP_CHECK(hipDeviceSynchronize());
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = bootstrap_weights_launch(L, seed, replicate, d, d + words, d + 2 * words, V, nullptr))) return rc;
    TRACS_HIP_CHECK(hipDeviceSynchronize());
    seconds[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    seconds[1] = seconds[2] = seconds[3] = 0.0;
    return gather_sites(var, d + 2 * words, out, n_out, nullptr, true, seconds + 1);      // (drains the stream before it returns)
}

// Host only.  A split is the bitset of an internal edge's child (tree_bitsets), turned to the side without leaf 0.  The replicate's
// splits are sorted by a hash; a main split counts when one of the candidates under its hash has the same words.
static uint64_t split_of(size_t n, const uint64_t *below, uint64_t *out)
{
    const size_t W = (n + 63) / 64;
    const bool flip = below[0] & 1ull;
    uint64_t h = 1469598103934665603ull;
    for (size_t w = 0; w < W; w++) {
        uint64_t x = flip ? ~below[w] : below[w];
        if (w + 1 == W && (n & 63)) x &= (1ull << (n & 63)) - 1ull;
        out[w] = x;
        h = (h ^ x) * 1099511628211ull;
        h ^= h >> 29;
    }
    return h;
}

int tracs_tree_support(size_t n, const uint32_t *parent, const uint32_t *child, size_t n_edges, const uint32_t *rep_parent,
                       const uint32_t *rep_child, size_t rep_n_edges, uint32_t *count)
{
    if (n < 4) return TRACS_OK;                                           // no internal edge
    if (!parent || !child || !rep_parent || !rep_child || !count) { set_error("tracs_tree_support: NULL argument"); return TRACS_E_ARG; }
    if (n > (1u << 24)) { set_error("tracs_tree_support: more than 2^24 leaves"); return TRACS_E_ARG; }
    const size_t W = (n + 63) / 64;
    std::vector<uint64_t> below_m, below_r;
    int rc;
    if ((rc = tree_bitsets("tracs_tree_support", n, parent, child, n_edges, &below_m, nullptr))) return rc;
    if ((rc = tree_bitsets("tracs_tree_support", n, rep_parent, rep_child, rep_n_edges, &below_r, nullptr))) return rc;
    // the replicate's splits, normalised in place of its bitsets (every internal node but the top one hangs on an internal edge)
    struct Key { uint64_t hash; size_t row; };
    std::vector<Key> keys;
    std::vector<uint64_t> tmp(W);
    for (size_t e = 0; e < rep_n_edges; e++) {
        if (rep_child[e] < n) continue;
        uint64_t *row = &below_r[(rep_child[e] - n) * W];
        const uint64_t h = split_of(n, row, tmp.data());
        std::memcpy(row, tmp.data(), W * 8);
        keys.push_back({h, (size_t)(rep_child[e] - n)});
    }
    std::sort(keys.begin(), keys.end(), [](const Key &a, const Key &b) { return a.hash < b.hash; });
    for (size_t e = 0; e < n_edges; e++) {
        if (child[e] < n) continue;
        const uint64_t h = split_of(n, &below_m[(child[e] - n) * W], tmp.data());
        auto it = std::lower_bound(keys.begin(), keys.end(), h, [](const Key &a, uint64_t v) { return a.hash < v; });
        for (; it != keys.end() && it->hash == h; ++it)
            if (std::memcmp(&below_r[it->row * W], tmp.data(), W * 8) == 0) { count[e] += 1; break; }
    }
    return TRACS_OK;
}

}  // extern "C"
